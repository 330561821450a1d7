"""Seeded inputs of the family sweep: ``draw(family, seed, limits)`` -> a dict of CPU tensors plus the drawn configuration.

Host only: no device tensor, no import of the library.  Deterministic in (family, seed, limits).  Sizes come from the
smallest values at which a kernel changes behaviour, never from the benchmark's workload; a value that is a constant
of the library (a chunk length, a per-graph limit) is passed in through ``limits`` by the caller, who reads it from the
library's own query.  Over a family's 16 seeds every listed boundary value, layout and route class is handed out at least
once BY CONSTRUCTION (:func:`_spread`): tests/test_fuzz_inputs.py asserts it against the lists below.

Every index is in range, every ``ptr`` is monotone, every edge of a batch stays inside its graph: nothing here is an
input a kernel is documented to reject.

Families: Just Balance ("jb"), DMoN's losses ("dmon"), HOSC's losses ("hosc"), AsymCheegerCut's losses ("acc"),
BN-Pool's reconstruction loss ("bnpool"), LaPool's selector ("lapool"), the segment readout ("readout"), the SAG scorer
("sag"), the k-MIS selector ("kmis"), the edge-contraction selector ("edge_contract"), ASAP's fitness ("asap") and
MaxCut's score net, cut loss and assignment rounds ("maxcut"), GTVConv's propagation with its two backward operators
("gtv"), PAN's MET matrix, its backward and the pooling score ("pan") and EigenPooling's modes, Reduce and Lift
("eigenpool").  New families are APPENDED: ``_gen`` seeds from a family's position in ``FAMILIES``.
"""
import os
import random
import sys

import torch

# The draws of "gtv" and "pan" depend on the float64 restatements (tests/gtv_restatement.py, tests/pan_restatement.py):
# their sub-seed walks ask the reference whether a candidate keeps its kinks or its top-k cut clear of rounding.  Those
# modules are imported inside the draw functions, from this directory.
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

FAMILIES = ("jb", "readout", "sag", "kmis", "edge_contract", "bnpool", "dmon", "hosc", "acc", "lapool", "asap", "maxcut",
            "gtv", "pan", "eigenpool")
SEEDS = tuple(range(16))

ROWS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
BATCHES = (1, 2, 5, 9)
CLUSTERS = (1, 2, 3, 7, 16, 17, 31, 32, 33, 64, 65)
FEATURES = (1, 3, 4, 5, 32, 33, 64, 67, 260)
DENSITIES = (0.0, 0.01, 0.2, 1.0)
ORDER_K = (1, 2, 3)
HUB_DEGREES = (65, 257)  # one in-degree past a wave, one past 256
# the two per-edge families (ASAP, MaxCut): one node's in-degree on either side of the 64-lane edge loops and past a
# multiple of every slot count; the list sorted by destination, by source, or shuffled (offsets only / a permutation, for
# the by-destination AND the by-source group)
EDGE_HUBS = (0, 63, 64, 65, 257)
EDGE_ORDERS = ("by_destination", "by_source", "shuffled")
# ASAP: in the 16-byte form G = 1, 2, 4, 8, 16, 32, 64 lanes share a row of ceil(F / 4) units (F = 4 | 5, 8 | 12, 16 |
# 17, 32 | 33, 64 | 67, 128 | 129 ...), and a second column block starts above 256 columns; one value per seed
ASAP_FEATURES = (1, 3, 4, 5, 8, 12, 16, 17, 32, 33, 64, 67, 128, 129, 257, 260)
ASAP_ACT_NAMES = ("identity", "tanh", "sigmoid")  # (the keys of kernels.ASAP_ACTS: tests/test_fuzz_inputs.py compares)
ASAP_QUERY_SCALE = 0.25  # the F x F Linear against 1 / sqrt(F) (see _draw_asap on the conditioning of the query half)
ASAP_LANES = {"vec16": (1, 2, 4, 8, 16, 32, 64), "scalar": (1, 4, 16, 64)}
MAXCUT_WIDTHS = (1, 2, 5, 8, 16, 31, 32, 33, 64)
MAXCUT_ACT_NAMES = ("identity", "tanh", "relu")  # (the keys of kernels.MAXCUT_ACTS)
MAXCUT_TAILS = ((), (16, 16), (64,), "unfit")  # "unfit": one mlp layer wider than the kernels' widest row
NP_CLASSES = ("full", "below", "empty", "loops")  # n_P = max(edge_index) + 1 against N; no edge; self-loops only
MAXCUT_KEEP = ("one", "half", "all")  # kept nodes per graph handed to the assignment rounds
FRAME_CACHE_ENTRIES = 4096  # a graph with more entries than this (and at most 1024 nodes) overflows the frame's LDS cache
# GTVConv (csrc/gtvconv.hip, ``gtv_pick``): G = 8 | 16 | 32 | 64 lanes own a node at C <= 32 | 64 | 128 | more, a lane holds
# R = 4 channels (8 above 256), a block of 256 threads holds 256 / G nodes, and above the library's register limit (512)
# the chunked kernels take one wave per node (4 per block).  16-byte loads at C % 4 == 0 on aligned rows, scalar loads
# otherwise: every switch has a width of either form on each side.  One value per seed.
GTV_WIDTHS = (1, 3, 4, 5, 32, 33, 64, 65, 128, 129, 256, 257, 260, 512, 513, 516)
GTV_LANE_GROUPS = ((32, 8, 4), (64, 16, 4), (128, 32, 4), (256, 64, 4))  # (widest C, G, R); wider rows: G = 64, R = 8
GTV_BATCHES = (1, 2, 3, 4, 5)
GTV_OUT_HUBS = (0, 1, 63, 64, 65)  # one node's out-degree (the forward's and the terms kernel's loop)
GTV_IN_HUBS = (0, 1, 65, 257)      # another node's in-degree, its out-degree 1: the node kernel's in-edge loop is the long one
GTV_ACT_NAMES = ("identity", "relu", "elu")  # (the keys of kernels.GTV_ACT_CODES)
GTV_DELTAS = (1.0, 0.311)
GTV_EPS = (1e-3, 0.5)  # the second clamps a share of the edges
GTV_MARGIN = 1e-4      # how far every kink of the propagation stays from the data (see _draw_gtv)
GTV_F_IN = 5           # input width of the public layer: h = x @ weight
GTV_SUB_SEEDS = 200
# PAN (csrc/pan.hip): the backward walks a row's stored entries 64 per step and a graph's columns 64 per step in a frame
# of max_n floats per wave; graphs of up to the library's limit (1024) nodes.  ``pan_score_kernel`` splits a node over
# G = 16 lanes (no query: the constant of that kernel), both for the F columns of x and for the node's column group.
PAN_SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129)
PAN_BATCHES = (1, 2, 5)
PAN_FILTERS = (0, 1, 2, 3, 4)
PAN_HUB_ENTRIES = (1, 63, 64, 65, 129)  # stored entries of one planted row
PAN_WEIGHTS = ("plain", "zero", "negative")  # |w| in [0.4, 0.9]; one exact zero; one negative
PAN_SCORE_LANES = 16
PAN_SCORE_FEATURES = (1, 15, 16, 17, 33, 64)
PAN_SCORE_GROUPS = (0, 1, 15, 16, 17, 33)  # entries of one node's column group
PAN_F = 4              # channels of x and of the convolution's output
PAN_GAP = 1e-4         # the kept and the dropped scores of every graph are at least this far apart
PAN_SUB_SEEDS = 200
# EigenPooling (csrc/eigenpool.hip).  The modes kernel solves groups of up to the library's limit (96) nodes; its rotation
# schedule pads odd sizes.  The Reduce kernel has no query for its constants: one wave adds a group of up to
# EIG_REDUCE_ONE_WAVE = 128 rows alone, 4 waves share longer ones up to EIG_REDUCE_FOUR_WAVES = 1024, 16 beyond (the host
# picks by the ``max_len`` hint), rows unrolled by 4, EIG_MODE_CHUNK = 8 modes per pass.
EIG_REDUCE_ONE_WAVE, EIG_REDUCE_FOUR_WAVES, EIG_MODE_CHUNK, EIG_ROW_UNROLL = 128, 1024, 8, 4
EIG_MODES = (1, 5, 8, 9)                  # H of the modes kernel
EIG_LONGEST = (127, 128, 129, 1023, 1024, 1025)  # rows of the Reduce's longest group
EIG_OTHER_ROWS = (0, 1, 5, 13)            # rows of its other groups
EIG_FEATURES = (1, 3, 63, 64, 65, 130)
EIG_REDUCE_MODES = (1, 7, 8, 9, 17)
EIG_K = 3                                 # clusters per graph of the modes draw
EIG_GAP = 1e-3                            # the spectral gap and the sign entry below which a group keeps the invariants only

# the limits each family reads from the library (name -> the rows drawn around it: L - 1, L, L + 1)
LIMITS = {
    "jb": ("part_rows",),
    "readout": ("segment_chunk_rows",),
    "sag": (),
    "kmis": ("kmis_max_graph_nodes",),
    "edge_contract": ("edge_contract_max_graph_nodes",),
    "bnpool": (),  # (its 32 x 32 logit tile: 31, 32, 33 are in ROWS)
    "dmon": ("part_rows",),
    "hosc": ("part_rows", "hosc_small_graph_nodes"),
    # (the 16 rows of a total-variation block and the 32 rows of its backward: 15 ... 17 and 31 ... 33 are in ROWS)
    "acc": ("acc_small_graph_nodes", "acc_tv_rows"),
    "lapool": (),
    "asap": (),
    "maxcut": (),
    "gtv": (),  # (graph sizes follow the nodes of a block at the drawn width, see _plan_gtv)
    "pan": ("pan_max_graph_nodes",),
    "eigenpool": ("eigenpool_max_group_nodes",),
}
# limits a draw reads without drawing graph sizes around them (the rows per partial sum of MaxCut's weight gradient,
# the widest row its kernels take; the widest row GTVConv's register kernels take)
DRAW_LIMITS = {"maxcut": ("maxcut_wgrad_rows", "maxcut_max_width"), "gtv": ("gtv_register_channels",)}
CLUSTER_LIMITS = {"bnpool": "bnpool_max_clusters"}  # K also draws this limit and half of it
LAYOUTS = {
    "jb": ("ptr", "ptr_offset", "sizes", "mask_prefix", "mask_holes", "mask_empty_row"),
    "readout": ("ptr", "ptr_sliced", "dense_plain", "dense_prefix", "dense_holes", "dense_empty_row", "gather",
                "gather_weighted"),
    "sag": ("plain", "sliced", "offset"),
    "kmis": ("graphs_sorted", "graphs_row_sorted", "plain_shuffled"),
    "edge_contract": ("graphs_sorted", "graphs_row_sorted", "plain_shuffled"),
    "bnpool": ("mask_none", "mask_prefix", "mask_holes", "mask_empty_row"),
    "dmon": ("mask_none", "mask_prefix", "mask_holes", "mask_empty_row", "sizes"),
    "hosc": ("mask_none", "mask_prefix", "mask_holes", "mask_empty_row", "sizes"),
    "acc": ("mask_none", "mask_prefix", "mask_holes", "mask_empty_row", "sizes"),
    "lapool": ("mask_none", "mask_prefix", "mask_holes", "mask_empty_row", "edges_sorted", "edges_shuffled",
               "edges_offset"),
    # x / x_pool as rows: contiguous; a column slice 4 bytes past a 16-byte boundary; a column slice that keeps the
    # 16-byte loads; contiguous but 4 bytes into its buffer
    "asap": ("plain", "sliced_unaligned", "sliced_aligned", "offset"),
    "maxcut": ("plain", "offset"),
    "gtv": ("plain", "offset"),  # h contiguous; contiguous but 4 bytes into its buffer (no 16-byte load may touch it)
    "pan": ("plain", "sliced"),  # the scorer's x: contiguous; a column slice (ldx > F)
    "eigenpool": ("plain", "sliced"),  # the Reduce's x: contiguous; a column slice
}
READOUT_OPS = ("sum", "mean", "min", "max")
READOUT_SUBSETS = tuple(tuple(op for i, op in enumerate(READOUT_OPS) if m >> i & 1) for m in range(1, 16))


def row_values(family, limits):
    """The rows-per-graph values of a family: ROWS plus L - 1, L, L + 1 of each of its limits."""
    vals = list(ROWS)
    for name in LIMITS[family]:
        lim = int(limits[name])
        vals += [v for v in (lim - 1, lim, lim + 1) if v not in vals]
    return vals


def cluster_values(family, limits):
    vals = list(CLUSTERS)
    if family in CLUSTER_LIMITS:
        lim = int(limits[CLUSTER_LIMITS[family]])
        vals += [v for v in (lim, lim // 2) if v not in vals]
    return vals


def _spread(values, counts, rng):
    """One list per seed with counts[s] entries: every value is handed out at least once (round-robin over the seeds
    that still have room, in a shuffled order), the rest of the room is filled with random picks."""
    vals = list(values)
    rng.shuffle(vals)
    out = [[] for _ in counts]
    i = 0
    while i < len(vals):
        before = i
        for s in range(len(counts)):
            if len(out[s]) < counts[s] and i < len(vals):
                out[s].append(vals[i])
                i += 1
        if i == before:
            raise ValueError(f"{len(vals)} values do not fit {sum(counts)} slots")
    for s in range(len(counts)):
        while len(out[s]) < counts[s]:
            out[s].append(rng.choice(vals))
    return out


def _one_each(values, rng, n=len(SEEDS)):
    return [v[0] for v in _spread(values, [1] * n, rng)]


_PLANS = {}


def plan(family, limits):
    """The 16 configurations of a family (cached): what each seed's draw must contain."""
    if family not in FAMILIES:
        raise ValueError(f"unknown family {family!r}")
    names = LIMITS[family] + ((CLUSTER_LIMITS[family],) if family in CLUSTER_LIMITS else ()) + DRAW_LIMITS.get(family, ())
    key = (family, tuple(sorted((k, int(v)) for k, v in limits.items() if k in names)))
    if key in _PLANS:
        return _PLANS[key]
    for attempt in range(1000):  # (the first plan that also holds the combinations _complete() asks for)
        cfgs = _plan(family, limits, random.Random(f"plan/{family}/{attempt}"))
        if _complete(family, limits, cfgs):
            _PLANS[key] = cfgs
            return cfgs
    raise RuntimeError(f"no complete plan for {family}")


def _complete(family, limits, cfgs):
    """Combinations the independent spreads do not guarantee: the all-false mask row sits in a batch of several graphs;
    for the selectors, the graph at the per-graph limit and
    the graph that overflows the edge cache must each meet the per-graph route at least once."""
    if any(c["layout"].endswith("empty_row") and c["B"] == 1 for c in cfgs):
        return False  # (the all-false row would be the whole batch: a draw that compares nothing)
    if family == "acc":  # a hub needs the un-padded form (real rows a prefix) and a graph to sit in; ties meet k > 1
        pre = ("mask_none", "mask_prefix", "sizes")
        return all(c["layout"] in pre and max(c["sizes"]) > 2 for c in cfgs if c["hub"]) \
            and any(c["ties"] and c["loss_k"] > 1 and max(c["sizes"]) > 8 for c in cfgs)
    if family == "hosc":  # the one-launch forward at its limit: N = the limit, K within it, the motif term on
        lim = int(limits["hosc_small_graph_nodes"])
        return any(max(c["sizes"]) == lim and c["K"] <= lim and c["alpha"] > 0 for c in cfgs)
    if family in ("asap", "maxcut"):
        return _complete_edges(family, cfgs)
    if family == "gtv":
        return _complete_gtv(limits, cfgs)
    if family == "pan":
        return _complete_pan(limits, cfgs)
    if family not in ("kmis", "edge_contract"):
        return True
    lim = int(limits[LIMITS[family][0]])
    on_graphs = [c for c in cfgs if c["layout"] != "plain_shuffled" and max(c["sizes"]) <= lim
                 and (c["density"] > 0 or c["big"])]
    return any(c["big"] for c in on_graphs) and any(max(c["sizes"]) == lim and c["density"] >= 0.2 for c in on_graphs)


def asap_row_geometry(f, layout):
    """(row stride in floats, byte offset of the first entry from a 16-byte boundary) of an [n, f] view in ``layout``."""
    return {"plain": (f, 0), "sliced_unaligned": (f + 3, 4), "sliced_aligned": ((f + 7) // 4 * 4, 0),
            "offset": (f, 4)}[layout]


def asap_load_form(f, layout):
    """"vec16" or "scalar": the row kernels' load form by the library's rule restated -- 16-byte loads when the row has
    at least 4 columns, its stride is a multiple of 4 floats and its first entry is 16-byte aligned."""
    stride, first = asap_row_geometry(f, layout)
    return "vec16" if f >= 4 and stride % 4 == 0 and first % 16 == 0 else "scalar"


def asap_lanes(f, form):
    """G, the lanes that share a row: the smallest listed count that holds the row's units (16-byte form: ceil(F / 4)
    float4 units; scalar form: F columns), 64 beyond."""
    units = -(-f // 4) if form == "vec16" else f
    return next((g for g in ASAP_LANES[form] if units <= g), 64)


def pow2_ceil(c):
    return 1 << max(c - 1, 0).bit_length()


def _complete_edges(family, cfgs):
    """ASAP / MaxCut: what forcing a value (no hub in a batch of tiny graphs, no hub without edges, a layout a width
    needs) may have taken away again, and the pairs the independent spreads do not guarantee."""
    if {c["hub"] for c in cfgs} != set(EDGE_HUBS) or {c["layout"] for c in cfgs} != set(LAYOUTS[family]):
        return False
    if family == "asap":
        form = {c["F"]: asap_load_form(c["F"], c["layout"]) for c in cfgs}  # (one seed per F)
        edges = {c["F"] for c in cfgs if c["hub"] or c["density"] >= 0.2}  # (a kernel that walks no edge shows nothing)
        if 260 not in edges:
            return False
        vec = {f for f, v in form.items() if v == "vec16"} & edges
        lanes = {asap_lanes(f, "vec16") for f in vec}
        return lanes == set(ASAP_LANES["vec16"]) and 8 in vec and bool({12, 16} & vec) and 32 in vec \
            and bool({257, 260} & vec) and form[260] == "scalar" \
            and {asap_lanes(f, "scalar") for f, v in form.items() if v == "scalar" and f in edges} == set(ASAP_LANES["scalar"])
    if {w for c in cfgs for w in c["widths"]} != set(MAXCUT_WIDTHS):
        return False
    pairs = [(a, b) for c in cfgs for a, b in zip(c["widths"][:-1], c["widths"][1:])]
    if not (any(b > a and pow2_ceil(b) != pow2_ceil(a) for a, b in pairs)
            and any(b < a and pow2_ceil(b) != pow2_ceil(a) for a, b in pairs)):
        return False
    if {c["np_class"] for c in cfgs} != set(NP_CLASSES) or not any(c["np_class"] == "below" and c["B"] > 1 for c in cfgs):
        return False
    return any(c["chain"] for c in cfgs) and any(c["tail"] == "unfit" for c in cfgs) \
        and any(c["weighted"] and c["np_class"] in ("full", "below") and c["density"] >= 0.2 for c in cfgs)


def _plan_edges(family, cfgs, rng):
    """The part of a plan ASAP and MaxCut share (the list), then each family's own."""
    for cfg, d, directed, weighted, order, hub in zip(cfgs, _one_each(DENSITIES, rng), _one_each((True, False), rng),
                                                      _one_each((True, False), rng), _one_each(EDGE_ORDERS, rng),
                                                      _one_each(EDGE_HUBS, rng)):
        # (a hub needs a graph to sit in: its sources are nodes of its own graph)
        cfg.update(density=d, directed=directed, weighted=weighted, order=order, hub=hub if max(cfg["sizes"]) > 2 else 0)
    if family == "asap":
        for cfg, f, slope, act, bias, same, mask, tied in zip(
                cfgs, _one_each(ASAP_FEATURES, rng), _one_each((0.2, 0.0), rng), _one_each(ASAP_ACT_NAMES, rng),
                _one_each((True, True, False), rng), _one_each((True, False), rng),
                _one_each((True, False, False, False), rng), _one_each((True, False, False, False), rng)):
            cfg.update(F=f, negative_slope=slope, act=act, bias=bias, same_pool=same, mask=mask, tied=tied)
            # the widths whose lane count or second column block must meet the 16-byte form get a layout that has it;
            # the widest meets the scalar form
            if f in (4, 8, 16, 32, 64, 128, 257):
                cfg["layout"] = rng.choice([lay for lay in LAYOUTS["asap"] if asap_load_form(f, lay) == "vec16"])
            elif f == 260:
                cfg["layout"] = rng.choice([lay for lay in LAYOUTS["asap"] if asap_load_form(f, lay) == "scalar"])
        return
    # (the input width F is not 1: the gradient to a 1 x 1 ``initial_layer`` is one sum of random signs over the nodes,
    # which float32 carries with whatever error its cancellation leaves)
    for cfg, depth, f, acts, delta, tail, npc, keep, max_iter, chain in zip(
            cfgs, _one_each((1, 2, 3, 4), rng), _one_each(MAXCUT_WIDTHS[1:], rng),
            zip(*(_one_each(MAXCUT_ACT_NAMES, rng) for _ in range(3))), _one_each((0.5, 2.0), rng),
            _one_each(MAXCUT_TAILS + MAXCUT_TAILS[:3], rng), _one_each(NP_CLASSES + ("full", "full", "below"), rng),
            _one_each(MAXCUT_KEEP + ("half",), rng), _one_each((1, 5), rng), _one_each((True, False, False, False), rng)):
        cfg.update(F=f, mp_act=acts[0], mlp_act=acts[1], act=acts[2], delta=delta, tail=tail, np_class=npc, keep=keep,
                   max_iter=max_iter, chain=chain and npc == "full")
        if npc in ("empty", "loops"):
            cfg["hub"] = 0
        widths = [rng.choice(MAXCUT_WIDTHS)]
        while len(widths) < depth:  # consecutive layers differ in width
            widths.append(rng.choice([w for w in MAXCUT_WIDTHS if w != widths[-1]]))
        cfg["widths"] = widths
    seen = {w for c in cfgs for w in c["widths"]}
    for w in MAXCUT_WIDTHS:  # every width is some layer's: the missing ones replace a repeated one
        if w not in seen:
            for c in cfgs:
                for i, old in enumerate(c["widths"]):
                    near = c["widths"][max(i - 1, 0):i] + c["widths"][i + 1:i + 2]
                    if w not in near and sum(old in o["widths"] for o in cfgs) > 1 and w not in seen:
                        c["widths"][i] = w
                        seen.add(w)


def gtv_layout_class(c, limits):
    """(G, R) of the register kernels at width ``c`` by the library's rule restated, "chunked" above its register limit."""
    if c > int(limits["gtv_register_channels"]):
        return "chunked"
    return next(((g, r) for top, g, r in GTV_LANE_GROUPS if c <= top), (64, 8))


def gtv_block_nodes(c, limits):
    """Nodes of one 256-thread block: 256 / G, one wave per node on the chunked kernels."""
    cls = gtv_layout_class(c, limits)
    return 4 if cls == "chunked" else 256 // cls[0]


def gtv_load_form(c, layout):
    """"vec16" (C % 4 == 0 on 16-byte aligned rows) or "scalar"; fresh outputs are aligned, so ``h`` decides."""
    return "vec16" if c % 4 == 0 and layout == "plain" else "scalar"


def _plan_gtv(limits, rng):
    """One width per seed; graph sizes P - 1, P, P + 1 around the P nodes of a block at that width, 1 and 2 besides; the
    widths that alone hold a lane group's 16-byte form keep aligned rows, 32 and 512 lose them."""
    n = len(SEEDS)
    cfgs = [{"family": "gtv", "seed": s, "C": c} for s, c in enumerate(_one_each(GTV_WIDTHS, rng))]
    batches = _one_each(GTV_BATCHES, rng)
    groups = {}
    for cfg in cfgs:
        cfg["block_nodes"] = gtv_block_nodes(cfg["C"], limits)
        groups.setdefault(cfg["block_nodes"], []).append(cfg)
    for p, group in sorted(groups.items()):
        need = -(-3 // len(group))  # graphs per seed so that P - 1, P and P + 1 all fit the group's seeds
        counts = [max(batches[c["seed"]], need) for c in group]
        small = (1, 2) if p == min(groups) else ()
        for cfg, b, sz in zip(group, counts, _spread((p - 1, p, p + 1) + small, counts, rng)):
            cfg["B"], cfg["sizes"] = b, list(sz)
    for cfg, out_hub, in_hub, order, loops, weighted, mask, lay, act, delta, eps, bias, dense in zip(
            cfgs, _one_each(GTV_OUT_HUBS, rng), _one_each(GTV_IN_HUBS, rng), _one_each(EDGE_ORDERS, rng),
            _one_each((True, False), rng), _one_each((True, False), rng), _one_each((True, False, False), rng),
            _one_each(LAYOUTS["gtv"], rng), _one_each(GTV_ACT_NAMES, rng), _one_each(GTV_DELTAS, rng),
            _one_each(GTV_EPS, rng), _one_each((True, True, True, False), rng), _one_each((True, True) + (False,) * 14, rng)):
        cfg.update(out_hub=out_hub, in_hub=in_hub, order=order, dups_loops=loops, weighted=weighted, mask=mask,
                   layout=lay, act=act, delta=delta, eps=eps, bias=bias, dense=dense, directed=rng.random() < 0.5)
        if cfg["C"] in (4, 64, 128, 256, 260):
            cfg["layout"] = "plain"
        elif cfg["C"] in (32, 512):
            cfg["layout"] = "offset"
    assert len(cfgs) == n
    return cfgs


def _complete_gtv(limits, cfgs):
    """Every graph-size value of every block size, a graph for the two hubs in every draw, every batch size, both load
    forms in every layout class of the register kernels, both layouts, and the pairs the spreads do not guarantee: relu
    with a mask and without, a long in-edge loop on either form of the by-destination index."""
    if {c["B"] for c in cfgs} != set(GTV_BATCHES) or {c["layout"] for c in cfgs} != set(LAYOUTS["gtv"]):
        return False
    if any(max(c["sizes"]) < 3 for c in cfgs) or not {1, 2} <= {v for c in cfgs for v in c["sizes"]}:
        return False
    for p in {c["block_nodes"] for c in cfgs}:
        if not {p - 1, p, p + 1} <= {v for c in cfgs if c["block_nodes"] == p for v in c["sizes"]}:
            return False
    forms = {(gtv_layout_class(c["C"], limits), gtv_load_form(c["C"], c["layout"])) for c in cfgs}
    classes = {k for k, _ in forms if k != "chunked"}
    if any((k, f) not in forms for k in classes for f in ("vec16", "scalar")):
        return False
    if {c["mask"] for c in cfgs if c["act"] == "relu"} != {True, False}:
        return False
    long_in = {c["order"] == "by_destination" for c in cfgs if c["in_hub"] >= 65}
    return long_in == {True, False} and any(c["eps"] == 0.5 and c["weighted"] for c in cfgs)


def _plan_pan(limits, rng):
    """Graph sizes 1 .. 129 and L - 1, L, L + 1 of the node limit over batches of 1, 2 and 5; a draw with a graph at the
    limit keeps filter_size <= 2 (and its big graphs a mean degree of 1.5); the planted row has one stored entry where
    filter_size = 0 leaves no other."""
    lim = int(limits["pan_max_graph_nodes"])
    batches = _one_each(PAN_BATCHES, rng)
    sizes = _spread(PAN_SIZES + (lim - 1, lim, lim + 1), batches, rng)
    seen = set()
    for sz in sizes:  # a size at the limit once over the seeds and alone in its draw: the random fill-ins become small ones
        for i, v in enumerate(sz):
            if v >= lim - 1 and (v in seen or any(u >= lim - 1 for u in sz[:i])):
                sz[i] = rng.choice(PAN_SIZES)
            elif v >= lim - 1:
                seen.add(v)
    cfgs = [{"family": "pan", "seed": s, "B": batches[s], "sizes": list(sizes[s])} for s in range(len(SEEDS))]
    for cfg, L, hub, kind, directed, order, lay, f, grp, use_tanh in zip(
            cfgs, _one_each(PAN_FILTERS * 3 + (2,), rng), _one_each(PAN_HUB_ENTRIES * 3 + (65,), rng), _one_each(PAN_WEIGHTS, rng),
            _one_each((True, False), rng), _one_each(("by_source", "shuffled"), rng), _one_each(LAYOUTS["pan"], rng),
            _one_each(PAN_SCORE_FEATURES, rng), _one_each(PAN_SCORE_GROUPS, rng), _one_each((True, False), rng)):
        big = max(cfg["sizes"]) >= lim - 1
        L = min(L, 2) if big else L
        cfg.update(filter_size=L, hub=hub if L > 0 else 1, weights=kind if L > 0 else "plain", directed=directed,
                   order=order, layout=lay, score_F=f, score_group=grp, use_tanh=use_tanh, at_limit=big)
    return cfgs


def _complete_pan(limits, cfgs):
    lim = int(limits["pan_max_graph_nodes"])
    if {c["hub"] for c in cfgs} != set(PAN_HUB_ENTRIES) or {c["filter_size"] for c in cfgs} != set(PAN_FILTERS):
        return False
    if {c["weights"] for c in cfgs} != set(PAN_WEIGHTS) or {c["B"] for c in cfgs} != set(PAN_BATCHES):
        return False
    # the three sizes at the limit in three draws (one reference of that size per draw); past a wave of stored entries
    # with the longest series; both list orders on the native route
    if not set(PAN_SIZES) | {lim - 1, lim, lim + 1} <= {v for c in cfgs for v in c["sizes"]}:
        return False
    if sum(c["at_limit"] for c in cfgs) != 3 or any(sum(v >= lim - 1 for v in c["sizes"]) > 1 for c in cfgs):
        return False
    if any(c["at_limit"] and c["filter_size"] == 0 for c in cfgs):  # (a series of one term shows nothing of a big graph)
        return False
    native = [c for c in cfgs if max(c["sizes"]) <= lim]
    return any(c["hub"] >= 65 and c["filter_size"] >= 3 for c in native) and {c["order"] for c in native} == {"by_source", "shuffled"} \
        and {c["directed"] for c in native} == {True, False}


EIG_SIZE_CLASSES = ("1", "2", "3", "H-1", "H", "H+1", "even", "odd", "L-1", "L", "L+1")


def _plan_eigenpool(limits, rng):
    """Modes: four group sizes per seed by class (1, 2, 3; around the drawn H; an even and an odd size in 20 .. 40;
    around the group limit), laid out as two graphs of EIG_K clusters -- [a, empty, b] and [c, d, 2].  Reduce and Lift:
    the longest group, the feature and mode counts, the layout of x."""
    lim = int(limits["eigenpool_max_group_nodes"])
    n = len(SEEDS)
    cfgs = []
    for s, (h, classes) in enumerate(zip(_one_each(EIG_MODES, rng), _spread(EIG_SIZE_CLASSES, [4] * n, rng))):
        size = {"1": 1, "2": 2, "3": 3, "H-1": max(h - 1, 1), "H": h, "H+1": h + 1, "even": 2 * rng.randrange(10, 21),
                "odd": 2 * rng.randrange(10, 20) + 1, "L-1": lim - 1, "L": lim, "L+1": lim + 1}
        a, b, c, e = (size[k] for k in classes)
        cfgs.append({"family": "eigenpool", "seed": s, "H": h, "classes": tuple(classes), "B": 2,
                     "sizes": [a + b, c + e + 2], "clusters": [[a, 0, b], [c, e, 2]]})
    for cfg, norm, longest, f, h2, lay in zip(cfgs, _one_each((True, False), rng), _one_each(EIG_LONGEST, rng),
                                              _one_each(EIG_FEATURES, rng), _one_each(EIG_REDUCE_MODES, rng),
                                              _one_each(LAYOUTS["eigenpool"], rng)):
        others = list(EIG_OTHER_ROWS) + [rng.choice(EIG_OTHER_ROWS), rng.choice(EIG_OTHER_ROWS)]
        rng.shuffle(others)
        cfg.update(normalized=norm, longest=longest, F=f, reduce_H=h2, layout=lay,
                   rows=others[:3] + [longest] + others[3:], hints=cfg["seed"] % 4 == 0)
    return cfgs


def _plan(family, limits, rng):
    n = len(SEEDS)
    if family == "gtv":
        return _plan_gtv(limits, rng)
    if family == "pan":
        return _plan_pan(limits, rng)
    if family == "eigenpool":
        return _plan_eigenpool(limits, rng)
    batches = _one_each(BATCHES, rng)
    # B >= 3: one slot is kept for the graph of 0 rows; 0 is not handed to the smaller batches (a batch without any row)
    counts = [b - 1 if b >= 3 else b for b in batches]
    sizes = _spread([v for v in row_values(family, limits) if v != 0], counts, rng)
    cfgs = []
    for s in range(n):
        sz = list(sizes[s])
        if batches[s] >= 3:
            sz.insert(rng.randrange(len(sz) + 1), 0)
        else:
            rng.shuffle(sz)
        cfgs.append({"family": family, "seed": s, "B": batches[s], "sizes": sz})
    for cfg, lay in zip(cfgs, _one_each(LAYOUTS[family], rng)):
        cfg["layout"] = lay
    if family == "jb":
        for cfg, k in zip(cfgs, _one_each(CLUSTERS, rng)):
            cfg["K"] = k
        for cfg, z in zip(cfgs, _one_each((True, False, False, False), rng)):
            cfg["zero_col"] = z and cfg["K"] > 1
        if not any(c["zero_col"] for c in cfgs):
            next(c for c in cfgs if c["K"] > 1)["zero_col"] = True
    elif family == "readout":
        for cfg, f, ops, integer in zip(cfgs, _one_each(FEATURES, rng), _one_each(READOUT_SUBSETS, rng),
                                        _one_each((True, False), rng)):
            cfg["F"], cfg["ops"], cfg["integer"] = f, ops, integer
    elif family == "sag":
        for cfg, f, d, w, mean, order, hub in zip(cfgs, _one_each(FEATURES, rng), _one_each(DENSITIES, rng),
                                                  _one_each((True, False), rng), _one_each((True, False), rng),
                                                  _one_each(("sorted", "shuffled"), rng),
                                                  _one_each(HUB_DEGREES + (0,), rng)):
            cfg.update(F=f, density=d, directed=w, mean=mean, order=order, hub=hub)
        for cfg, root, bias in zip(cfgs, _one_each((True, True, False), rng), _one_each((True, False), rng)):
            cfg["root"], cfg["bias"] = root, bias
    elif family == "lapool":
        for cfg, f, d, directed, weighted in zip(cfgs, _one_each(FEATURES, rng), _one_each(DENSITIES, rng),
                                                 _one_each((True, False), rng), _one_each((True, False), rng)):
            cfg.update(F=f, density=d, directed=directed, weighted=weighted)
    elif family in ("dmon", "hosc", "acc"):
        for cfg, k, d, directed, weighted in zip(cfgs, _one_each(CLUSTERS, rng), _one_each(DENSITIES, rng),
                                                 _one_each((True, False), rng), _one_each((True, False), rng)):
            cfg.update(K=k, density=d, directed=directed, weighted=weighted)
        if family == "acc":  # the loss's k, exactly tied entries in S's columns, a hub past a wave / past 256 in-edges
            for cfg, k, ties, hub in zip(cfgs, _one_each((1, 2, 3, 7), rng), _one_each((True, False), rng),
                                         _one_each(HUB_DEGREES + (0, 0), rng)):
                cfg.update(loss_k=k, ties=ties, hub=hub)
        if family == "hosc":  # the weights of the two cuts, which orthogonality term, trace(S^T A S) given or not
            for cfg, alpha, ho, raw in zip(cfgs, _one_each((0.0, 0.5, 1.0), rng), _one_each((True, False), rng),
                                           _one_each((True, False), rng)):
                cfg.update(alpha=alpha, mu=0.7, hosc_ortho=ho, with_raw=raw)
    elif family == "bnpool":
        for cfg, k, d, directed, weighted in zip(cfgs, _one_each(cluster_values(family, limits), rng),
                                                 _one_each(DENSITIES, rng), _one_each((True, False), rng),
                                                 _one_each((True, False), rng)):
            cfg.update(K=k, density=d, directed=directed, weighted=weighted)
    elif family in ("asap", "maxcut"):
        _plan_edges(family, cfgs, rng)
    else:  # the two selectors
        for cfg, d, directed, big in zip(cfgs, _one_each(DENSITIES, rng), _one_each((True, False), rng),
                                         _one_each((True, False, False, False), rng)):
            cfg.update(density=d, directed=directed, big=big)
            if family == "kmis":
                cfg["order_k"] = None
        if family == "kmis":
            for cfg, k in zip(cfgs, _one_each(ORDER_K, rng)):
                cfg["order_k"] = k
    return cfgs


# ------------------------------------------------------------------------------------------------------------ helpers
def _gen(family, seed):
    g = torch.Generator()
    g.manual_seed(1_000_003 * (FAMILIES.index(family) + 1) + seed)
    return g


def _ptr(sizes):
    p = torch.zeros(len(sizes) + 1, dtype=torch.long)
    p[1:] = torch.tensor(sizes, dtype=torch.long).cumsum(0)
    return p


def _batch(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))


def _edges(n, density, directed, g, self_loops=True, duplicates=True, isolated=True):
    """Edge entries [2, E] of one graph (local ids, list order random): density 0 gives none, 1 the full graph."""
    if n == 0 or density == 0.0:
        return torch.zeros(2, 0, dtype=torch.long)
    a = torch.rand(n, n, generator=g) < density
    if not directed:
        a = torch.triu(a, 1)
        a = a | a.t()
    else:
        a.fill_diagonal_(False)
    if self_loops and n > 2:
        a[n // 3, n // 3] = True
    if isolated and n > 4 and density < 1.0:
        a[n // 2, :] = False
        a[:, n // 2] = False
    e = a.nonzero().t()
    if duplicates and e.size(1) > 2:
        e = torch.cat([e, e[:, : max(1, e.size(1) // 7)]], 1)
    return e[:, torch.randperm(e.size(1), generator=g)].contiguous()


def _order(ei, how, n):
    """"sorted": by (row, col), stable; "row_sorted": sources ascend, targets in drawn order; "shuffled": as drawn."""
    if how == "shuffled" or ei.size(1) == 0:
        return ei
    key = ei[0] * max(n, 1) + ei[1] if how == "sorted" else ei[0]
    return ei[:, torch.argsort(key, stable=True)].contiguous()


def _assignment(sizes, k, g, zero_col):
    n = sum(sizes)
    s = torch.softmax(2 * torch.randn(n, k, generator=g), -1) if k > 1 else torch.rand(n, 1, generator=g)
    if zero_col:
        s[:, k // 2] = 0.0
    return s


def _pad(rows, sizes, n):
    out = torch.zeros((len(sizes), n) + tuple(rows.shape[1:]), dtype=rows.dtype)
    off = 0
    for b, c in enumerate(sizes):
        out[b, :c] = rows[off:off + c]
        off += c
    return out


def _masks(sizes, n, kind, g):
    prefix = torch.arange(n).view(1, -1) < torch.tensor(sizes).view(-1, 1)
    if kind == "prefix":
        return prefix
    holes = torch.rand(len(sizes), n, generator=g) < 0.6
    holes[0, : min(n, 1)] = True
    if kind == "empty_row":
        holes[len(sizes) // 2] = False
    return holes


# ------------------------------------------------------------------------------------------------------------ families
def _draw_jb(cfg, g, limits):
    sizes, k, lay = cfg["sizes"], cfg["K"], cfg["layout"]
    n = max(sizes)
    d = dict(cfg)
    d["N"], d["ptr"], d["batch"] = n, _ptr(sizes), _batch(sizes)
    if lay in ("mask_holes", "mask_empty_row"):
        # the public padded form: EVERY row of S counts, the mask only gives n_b (it has holes; one row all false)
        d["s"] = _assignment([n] * len(sizes), k, g, cfg["zero_col"]).view(len(sizes), n, k)
        d["mask"] = _masks(sizes, n, "holes" if lay == "mask_holes" else "empty_row", g)
        d["n_b"] = d["mask"].sum(1).tolist()
        d["padded"] = True
    else:
        flat = _assignment(sizes, k, g, cfg["zero_col"])
        d["s_flat"], d["s_padded"] = flat, _pad(flat, sizes, n)
        d["mask"] = _masks(sizes, n, "prefix", g)
        d["n_b"] = list(sizes)
        d["padded"] = lay in ("sizes", "mask_prefix")
        d["s"] = d["s_padded"] if d["padded"] else flat
    return d


def _draw_readout(cfg, g, limits):
    sizes, f, lay = cfg["sizes"], cfg["F"], cfg["layout"]
    d = dict(cfg)
    b = len(sizes)

    def values(*shape):
        if cfg["integer"]:
            return torch.randint(-2, 3, shape, generator=g).float()
        return torch.randn(*shape, generator=g)

    if lay in ("ptr", "ptr_sliced"):
        rows = sum(sizes)
        if lay == "ptr_sliced":  # a column slice with a row stride of its own (first column 1: rows off by 4 bytes)
            d["x_base"], d["first"] = values(rows, f + 7), 1
            d["x"] = d["x_base"][:, 1:1 + f]
        else:
            d["x"] = values(rows, f)
        d["ptr"], d["batch"], d["groups"], d["max_len"] = _ptr(sizes), _batch(sizes), b, max(sizes)
        d["index"] = d["batch"]
        d["src_rows"] = torch.arange(rows)
    elif lay.startswith("dense"):
        n = max(sizes)
        d["N"], d["x"] = n, values(b, n, f)
        kind = lay.split("_", 1)[1]
        d["mask"] = None if kind == "plain" else _masks(sizes, n, kind, g)
        keep = torch.ones(b * n, dtype=torch.bool) if d["mask"] is None else d["mask"].reshape(-1)
        d["index"] = torch.arange(b).repeat_interleave(n)[keep]
        d["src_rows"] = keep.nonzero().view(-1)
        d["groups"], d["max_len"] = b, n
    else:  # a sparse assignment: supernode c owns sizes[c] of the kept nodes
        kept = sum(sizes)
        nodes = kept + 5
        d["x"] = values(nodes, f)
        d["node_index"] = torch.randperm(nodes, generator=g)[:kept].sort().values
        d["cluster_index"] = _batch(sizes)[torch.randperm(kept, generator=g)]
        d["weight"] = None
        if lay == "gather_weighted":
            d["weight"] = (torch.randint(1, 3, (kept,), generator=g).float() if cfg["integer"]
                           else torch.rand(kept, generator=g) + 0.1)
        d["num_nodes"], d["groups"], d["max_len"] = nodes, b, max(sizes)
        d["index"], d["src_rows"] = d["cluster_index"], d["node_index"]
    return d


def _draw_sag(cfg, g, limits):
    sizes, f = cfg["sizes"], cfg["F"]
    d = dict(cfg)
    ptr = _ptr(sizes)
    n = int(ptr[-1])
    parts = [_edges(c, cfg["density"], cfg["directed"], g) + int(ptr[i]) for i, c in enumerate(sizes)]
    ei = torch.cat(parts, 1) if parts else torch.zeros(2, 0, dtype=torch.long)
    if cfg["hub"] and n > 1:  # one node whose in-degree is past a wave / past 256 (sources repeat: duplicates)
        hub = n // 2
        src = torch.randint(0, n, (cfg["hub"],), generator=g)
        ei = torch.cat([ei, torch.stack([src, torch.full_like(src, hub)])], 1)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    if cfg["order"] == "sorted":  # ascending destinations: the scorer reads the list's own CSR offsets
        ei = ei[:, torch.argsort(ei[1], stable=True)]
    d["edge_index"], d["n"] = ei.contiguous(), n
    d["in_degree_max"] = int(torch.bincount(ei[1], minlength=max(n, 1)).max()) if ei.size(1) else 0
    lay = cfg["layout"]
    if lay == "sliced":
        d["x_base"], d["first"] = torch.randn(n, f + 5, generator=g), 2
        d["x"] = d["x_base"][:, 2:2 + f]
    else:
        d["x"] = torch.randn(n, f, generator=g)
    scale = 1.0 / max(f, 1) ** 0.5
    d["w_rel"] = torch.randn(1, f, generator=g) * scale
    d["w_root"] = torch.randn(1, f, generator=g) * scale if cfg["root"] else None
    d["b"] = torch.randn(1, generator=g) if cfg["bias"] else None
    return d


def _draw_selector(cfg, g, limits):
    d = dict(cfg)
    sizes = list(cfg["sizes"])
    dens = [cfg["density"]] * len(sizes)
    if cfg["big"]:  # a graph of at most 1024 nodes with more than 4096 entries, between the others
        at = len(sizes) // 2
        sizes.insert(at, 600)
        dens.insert(at, 0.02)
    ptr = _ptr(sizes)
    n = int(ptr[-1])
    parts = []
    for i, (c, den) in enumerate(zip(sizes, dens)):
        if c > 256 and den > 0.03:
            den = 0.03  # the full graph of a 1000-node limit case would be a million entries
        parts.append(_edges(c, den, cfg["directed"], g) + int(ptr[i]))
    ei = torch.cat(parts, 1)
    if cfg["big"]:
        lo, hi = int(ptr[at]), int(ptr[at + 1])
        own = int(((ei[0] >= lo) & (ei[0] < hi)).sum())
        assert own > FRAME_CACHE_ENTRIES, own
        d["big_entries"] = own
    lay = cfg["layout"]
    if lay == "plain_shuffled":
        ei = ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()
        d["graph_ptr"], d["max_graph_nodes"] = None, None
    else:
        ei = _order(ei, "sorted" if lay == "graphs_sorted" else "row_sorted", n)
        d["graph_ptr"], d["max_graph_nodes"] = ptr, max(sizes)
    d["all_sizes"], d["n"], d["edge_index"] = sizes, n, ei
    items = n if cfg["family"] == "kmis" else ei.size(1)
    # the per-graph route: a sorted batch (sources ascend) whose longest graph fits the library's limit; the edge
    # contraction also needs an entry to match
    fits = lay != "plain_shuffled" and max(sizes) <= int(limits[LIMITS[cfg["family"]][0]])
    if cfg["family"] == "edge_contract" and ei.size(1) == 0:
        fits = False
    d["route"] = "graphs" if fits else "rounds"
    d["perm"] = torch.randperm(items, generator=g)
    # small integers as scores: most entries are exactly tied, so the rule "the lower index goes first" decides the
    # order and no float comparison is open
    d["score"] = torch.randint(0, 6, (items,), generator=g).float()
    return d


def _draw_bnpool(cfg, g, limits):
    """S [B,N,K], the cluster matrix [K,K], adj [B,N,N] (weighted or 0/1, symmetric or directed) and the mask.  Under
    "mask_prefix" everything outside the mask is zero, as densification leaves it; under the masks with holes S and adj
    keep their values there: the mask alone must decide."""
    sizes, k, lay = cfg["sizes"], cfg["K"], cfg["layout"]
    b, n = len(sizes), max(sizes)
    d = dict(cfg)
    d["N"] = n
    s = _assignment([n] * b, k, g, False).view(b, n, k)
    a = (torch.rand(b, n, n, generator=g) < cfg["density"]).float()
    if cfg["weighted"]:
        a = a * (torch.rand(b, n, n, generator=g) + 0.25)
    if not cfg["directed"]:
        a = torch.triu(a, 1)
        a = a + a.transpose(1, 2)
    if lay == "mask_none":
        d["mask"], d["n_b"] = None, [n] * b
    else:
        d["mask"] = _masks(sizes, n, {"mask_prefix": "prefix", "mask_holes": "holes", "mask_empty_row": "empty_row"}[lay], g)
        d["n_b"] = d["mask"].sum(1).tolist()
        if lay == "mask_prefix":
            s = s * d["mask"].unsqueeze(-1)
            a = a * d["mask"].unsqueeze(1) * d["mask"].unsqueeze(2)
    d["s"], d["adj"] = s.contiguous(), a.contiguous()
    d["k_mat"] = torch.randn(k, k, generator=g)
    return d


def _draw_dmon(cfg, g, limits):
    """S [B,N,K] (zero outside the mask, as the selector leaves it), adj [B,N,N] (zero outside the mask, as densification
    leaves it), the mask and the graph sizes; the same batch un-padded (rows, ptr, a row-sorted edge list with its
    per-graph edge offsets) where the real rows are a prefix.

    Conditioning.  Both the spectral term (trace / 2m against ||S^T d||^2 / 4m^2) and the cluster term (||S^T 1|| sqrt(K)
    / n against 1) are differences that vanish for a balanced, structure-free draw, where float32 has nothing left to
    compare.  So every graph has planted communities of unequal sizes, S is a softmax peaked on a node's community
    (cluster term well above 0) and the weights of edges across communities are a tenth of those inside (modularity well
    above 0); an unweighted draw keeps 0/1 entries and drops three cross-community edges in four instead."""
    sizes, k, lay = cfg["sizes"], cfg["K"], cfg["layout"]
    b, n = len(sizes), max(sizes)
    d = dict(cfg)
    d["N"] = n
    if lay == "mask_none":
        mask = torch.ones(b, n, dtype=torch.bool)
    else:
        kind = {"mask_prefix": "prefix", "sizes": "prefix", "mask_holes": "holes", "mask_empty_row": "empty_row"}[lay]
        mask = _masks(sizes, n, kind, g)
    d["real"] = mask  # the rows that count
    d["mask"] = None if lay == "mask_none" else mask
    d["graph_sizes"] = torch.tensor(sizes) if lay == "sizes" else None  # (a hint to skip the padding; n_b is the mask's)
    d["n_b"] = mask.sum(1).tolist()
    prob = torch.arange(1, k + 1, dtype=torch.float32) ** 2
    comm = torch.multinomial(prob / prob.sum(), b * n, replacement=True, generator=g).view(b, n)
    logits = torch.randn(b, n, k, generator=g) + 4.0 * torch.nn.functional.one_hot(comm, k)
    s = (torch.softmax(logits, -1) if k > 1 else torch.rand(b, n, 1, generator=g)) * mask.unsqueeze(-1)
    a = (torch.rand(b, n, n, generator=g) < cfg["density"]).float()
    same = comm.unsqueeze(1) == comm.unsqueeze(2)
    if cfg["weighted"]:
        a = a * (torch.rand(b, n, n, generator=g) + 0.25) * torch.where(same, 1.0, 0.1)
    else:
        a = a * (same | (torch.rand(b, n, n, generator=g) < 0.25)).float()
    if not cfg["directed"]:
        a = torch.triu(a, 1)
        a = a + a.transpose(1, 2)
    a = a * mask.unsqueeze(1) * mask.unsqueeze(2)
    d["s"], d["adj"] = s.contiguous(), a.contiguous()
    d["prefix"] = lay in ("mask_none", "mask_prefix", "sizes")
    if d["prefix"]:
        rows = d["n_b"]
        d["ptr"], d["batch"] = _ptr(rows), _batch(rows)
        d["s_flat"] = torch.cat([s[i, :c] for i, c in enumerate(rows)])
        ei, w, eptr = [], [], [0]
        for i in range(b):
            e = a[i].nonzero().t()  # (row-major: the sources ascend)
            ei.append(e + int(d["ptr"][i]))
            w.append(a[i][e[0], e[1]])
            eptr.append(eptr[-1] + e.size(1))
        d["edge_index"], d["edge_weight"] = torch.cat(ei, 1).contiguous(), torch.cat(w)
        d["edge_ptr"] = torch.tensor(eptr)
        d["n"], d["all_sizes"] = int(d["ptr"][-1]), list(rows)
    return d


def _draw_acc(cfg, g, limits):
    """DMoN's batch (S, adj, mask / sizes, the un-padded form) with, where drawn, a share of exactly tied entries in
    every column of S (values on a grid of eighths: the rule "the lowest row holds the quantile" must decide) and, on
    the edge form, one node whose in-degree is past a wave or past 256 (its sources repeat: duplicates; the list is no
    longer sorted)."""
    d = _draw_dmon(cfg, g, limits)
    if cfg["ties"]:
        d["s"] = (torch.round(d["s"] * 8) / 8).contiguous()
        if d["prefix"]:
            d["s_flat"] = torch.cat([d["s"][i, :c] for i, c in enumerate(d["n_b"])])
    d["in_degree_max"] = 0
    if d["prefix"]:
        if not cfg["weighted"]:
            d["edge_weight"] = None
        if cfg["hub"]:
            big = max(range(len(d["n_b"])), key=lambda i: d["n_b"][i])
            lo, n = int(d["ptr"][big]), d["n_b"][big]
            src = torch.randint(0, n, (cfg["hub"],), generator=g) + lo
            extra = torch.stack([src, torch.full_like(src, lo + n // 2)])
            d["edge_index"] = torch.cat([d["edge_index"], extra], 1).contiguous()
            if d["edge_weight"] is not None:
                d["edge_weight"] = torch.cat([d["edge_weight"], torch.rand(cfg["hub"], generator=g) + 0.25])
        if d["edge_index"].size(1):
            d["in_degree_max"] = int(torch.bincount(d["edge_index"][1]).max())
    return d


def _draw_lapool(cfg, g, limits):
    """Padded: x [B,N,F], adj [B,N,N], a mask (under the masks with holes x and adj keep their values outside it: the
    mask alone must decide).  Edge list: x [n,F], a sorted batch, entries with self-loops, duplicates, isolated nodes
    and (weighted) explicit zero weights, sources ascending or shuffled.  ``v_tied``: integer-valued variations, so the
    leader rule v_i >= v_j is decided on exact ties."""
    sizes, f, lay = cfg["sizes"], cfg["F"], cfg["layout"]
    b, n = len(sizes), max(sizes)
    d = dict(cfg)
    d["padded"] = lay.startswith("mask")
    if d["padded"]:
        d["N"] = n
        kind = lay.split("_", 1)[1]
        d["mask"] = None if kind == "none" else _masks(sizes, n, kind, g)
        real = torch.ones(b, n, dtype=torch.bool) if d["mask"] is None else d["mask"]
        x = torch.randn(b, n, f, generator=g)
        a = (torch.rand(b, n, n, generator=g) < cfg["density"]).float()
        if cfg["weighted"]:
            a = a * (torch.rand(b, n, n, generator=g) + 0.25)
        if not cfg["directed"]:
            a = torch.triu(a, 1)
            a = a + a.transpose(1, 2)
        if kind == "prefix":
            x, a = x * real.unsqueeze(-1), a * real.unsqueeze(1) * real.unsqueeze(2)
        d["x"], d["adj"], d["real"] = x.contiguous(), a.contiguous(), real
        d["n_b"] = real.sum(1).tolist()
        d["v_tied"] = torch.randint(0, 4, (b, n), generator=g).float()
    else:
        ptr = _ptr(sizes)
        total = int(ptr[-1])
        parts = [_edges(c, cfg["density"], cfg["directed"], g) + int(ptr[i]) for i, c in enumerate(sizes)]
        ei = torch.cat(parts, 1)
        if lay != "edges_shuffled":
            ei = _order(ei, "row_sorted", total)
        d["edge_index"], d["n"] = ei.contiguous(), total
        d["edge_weight"] = None
        if cfg["weighted"]:
            w = torch.rand(ei.size(1), generator=g) + 0.25
            w[::5] = 0.0  # explicit zero weights: still neighbours for the leader rule
            d["edge_weight"] = w
        d["x"] = torch.randn(total, f, generator=g)
        d["ptr"], d["batch"], d["n_b"] = ptr, _batch(sizes), list(sizes)
        d["v_tied"] = torch.randint(0, 4, (total,), generator=g).float()
    return d


def _edge_list(cfg, g, sizes, np_class=None, chain=0):
    """The batch's list for ASAP and MaxCut -> (edge_index [2,E], edge_weight or None, ptr, n, every graph's size).

    Per graph `_edges` (self-loops, duplicates, an isolated node; graphs above 64 nodes are thinned to an average degree
    of at most 16, so that a float64 run of the reference stays small).  ``np_class`` (MaxCut): "empty" no edge at all,
    "loops" self-loops only (some twice), "below" the last two nodes of the batch above every endpoint, "full" the last
    node an endpoint.  The hub: one node of the longest graph whose in-degree is EXACTLY ``cfg["hub"]``, its sources
    drawn with repeats from its own graph.  ``chain``: one more graph at the end, a directed path of that many nodes.
    Then the whole list is shuffled and put into the drawn order; about a tenth of the weights are exactly 0."""
    sizes = list(sizes) + ([chain] if chain else [])
    ptr = _ptr(sizes)
    n = int(ptr[-1])
    parts = []
    for i, c in enumerate(sizes[:len(cfg["sizes"])]):
        den = cfg["density"] if c <= 64 else min(cfg["density"], 16.0 / c)
        parts.append(_edges(c, den, cfg["directed"], g) + int(ptr[i]))
    ei = torch.cat(parts, 1)
    top = n
    if np_class == "empty":
        ei = ei[:, :0]
    elif np_class == "loops":
        loop = torch.randint(0, n, (max(1, n // 2),), generator=g)
        loop = torch.cat([loop, loop[: max(1, loop.numel() // 3)]])
        ei = torch.stack([loop, loop])
    elif np_class == "below" and n > 2:
        top = n - 2
        ei = ei[:, (ei < top).all(0)]
    if cfg["hub"]:
        big = max(range(len(cfg["sizes"])), key=lambda i: sizes[i])
        lo, c = int(ptr[big]), sizes[big]
        hi = min(lo + c, top)
        node = min(lo + c // 2, hi - 1)
        src = torch.randint(lo, hi, (cfg["hub"],), generator=g)
        ei = torch.cat([ei[:, ei[1] != node], torch.stack([src, torch.full_like(src, node)])], 1)
    if chain:
        path = torch.arange(n - chain, n - 1)
        ei = torch.cat([ei, torch.stack([path, path + 1])], 1)
    if np_class == "full" and (ei.numel() == 0 or int(ei.max()) < n - 1):
        last = n - 1 - (1 if sizes[-1] > 1 else 0)  # (an edge inside the last graph, a self-loop where it has one node)
        ei = torch.cat([ei, torch.tensor([[last], [n - 1]])], 1)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    if cfg["order"] != "shuffled":
        ei = ei[:, torch.argsort(ei[1 if cfg["order"] == "by_destination" else 0], stable=True)]
    ew = None
    if cfg["weighted"]:
        ew = torch.rand(ei.size(1), generator=g) + 0.25
        ew[torch.rand(ei.size(1), generator=g) < 0.1] = 0.0
    return ei.contiguous(), ew, ptr, n, sizes


def _distinct_rows(n, f, g):
    """[n, f] in (-2, 2) with no two equal entries in a column: arg-max ties between DIFFERENT rows cannot occur (the
    kernel keeps the lower edge position, torch's amax backward splits the gradient: the two agree only on duplicates)."""
    if n == 0:
        return torch.zeros(0, f)
    rank = torch.argsort(torch.rand(n, f, generator=g), dim=0).float()
    return ((rank + 0.25 + 0.5 * torch.rand(n, f, generator=g)) * (4.0 / n) - 2.0).contiguous()


def _draw_asap(cfg, g, limits):
    """x and x_pool [n, F] (x_pool the same tensor or its own), the list (`_edge_list`), the parameters of the attention
    (``lin`` F x F, ``att`` 2F -> 1) and of the one-channel LEConv under the restatement's names (a bias that is off is
    None), a dropout-style ``mask`` on alpha where drawn, and where drawn ``x_tied``: x_pool on a grid of halves, so that
    most maxima are held by several different source rows (forward only: the exact arg-max positions)."""
    f = cfg["F"]
    d = dict(cfg)
    ei, ew, ptr, n, sizes = _edge_list(cfg, g, cfg["sizes"])
    d.update(edge_index=ei, edge_weight=ew, ptr=ptr, n=n, batch=_batch(sizes))
    d["in_degree_max"] = int(torch.bincount(ei[1], minlength=1).max()) if ei.size(1) else 0
    d["form"] = asap_load_form(f, cfg["layout"])
    d["lanes"] = asap_lanes(f, d["form"])
    d["x"] = _distinct_rows(n, f, g)
    d["x_pool"] = d["x"] if cfg["same_pool"] else _distinct_rows(n, f, g)
    d["x_tied"] = (torch.round(d["x_pool"] * 2) / 2).contiguous() if cfg["tied"] else None
    scale = 1.0 / f ** 0.5
    # (the softmax of a group does not see a shift of all its logits, and leaky(sq_i + sp_j) shifts a whole group by sq_i
    # unless its logits straddle 0: the query half is kept small against the source half, so that most groups with
    # several edges do straddle it and the gradient to sq, lin and the biases is more than rounding noise around 0)
    par = {"lin.weight": torch.randn(f, f, generator=g) * (ASAP_QUERY_SCALE * scale),
           "lin.bias": torch.randn(f, generator=g) * 0.1,
           "att.weight": torch.randn(1, 2 * f, generator=g) * scale, "att.bias": torch.randn(1, generator=g) * 0.1}
    # (LEConv sums w_e (lin1(x_src) - lin2(x_i)) over a group: lin1, lin2 and lin1's bias are a tenth and a thirtieth of
    # the rest, so that a hub of 257 in-edges still lands where tanh and sigmoid are not saturated)
    for k in (1, 2, 3):
        par[f"select_scorer.lin{k}.weight"] = torch.randn(1, f, generator=g) * (scale if k == 3 else 0.1 * scale)
    par["select_scorer.lin1.bias"] = torch.randn(1, generator=g) * 0.01
    par["select_scorer.lin3.bias"] = torch.randn(1, generator=g) * 0.3
    if not cfg["bias"]:
        par = {k: (None if k.endswith("bias") else v) for k, v in par.items()}
    d["params"] = par
    d["alpha_mask"] = None
    if cfg["mask"]:
        d["alpha_mask"] = (torch.rand(ei.size(1), generator=g) > 0.3).float() / 0.7
    return d


def _draw_maxcut(cfg, g, limits):
    """x [n, F], the list with its ``n_P`` class, the score net's parameters under the reference's names (widths F ->
    ``widths`` -> ``tail`` -> 1), scores ``s`` in (0.1, 0.9) for the cut loss (one sign: s^T A s / vol cannot cancel),
    the kept nodes for the assignment rounds (1 .. all per graph, sorted) and, where drawn, a directed path longer than
    ``max_iter`` as one more graph with only its head kept.  With weights, one node's out-edges all weigh 0: its degree
    is 0 although it has edges."""
    pre = "selector.score_net."
    d = dict(cfg)
    chain = cfg["max_iter"] + 4 if cfg["chain"] else 0
    ei, ew, ptr, n, sizes = _edge_list(cfg, g, cfg["sizes"], cfg["np_class"], chain)
    d["zero_degree_node"] = None
    if ew is not None:
        cand = ei[0][ei[0] != ei[1]]
        if cand.numel():
            v = int(cand[int(torch.randint(0, cand.numel(), (1,), generator=g))])
            ew[ei[0] == v] = 0.0
            d["zero_degree_node"] = v
    d.update(edge_index=ei, edge_weight=ew, ptr=ptr, n=n, all_sizes=sizes, batch=_batch(sizes))
    d["n_p"] = int(ei.max()) + 1 if ei.numel() else 0
    d["in_degree_max"] = int(torch.bincount(ei[1], minlength=1).max()) if ei.size(1) else 0
    f, widths = cfg["F"], cfg["widths"]
    d["x"] = torch.randn(n, f, generator=g)
    tail = (2 * int(limits["maxcut_max_width"]),) if cfg["tail"] == "unfit" else tuple(cfg["tail"])
    d["mlp_units"] = list(tail)

    def linear(name, out, inp, par):
        par[pre + name + ".weight"] = torch.randn(out, inp, generator=g) / inp ** 0.5
        par[pre + name.replace(".lin", "") + ".bias"] = torch.randn(out, generator=g) * 0.3
    par = {}
    linear("initial_layer", f, f, par)
    for l, (i, o) in enumerate(zip([f] + widths[:-1], widths)):
        linear(f"mp_convs.{l}.lin", o, i, par)
    for l, (i, o) in enumerate(zip([widths[-1]] + list(tail[:-1]), tail)):
        linear(f"mlp.{l}", o, i, par)
    linear("final_layer", 1, tail[-1] if tail else widths[-1], par)
    d["params"] = par
    d["cfg"] = dict(mp_units=list(widths), mlp_units=list(tail), mp_act=cfg["mp_act"], mlp_act=cfg["mlp_act"],
                    act=cfg["act"], delta=cfg["delta"])
    d["s"] = 0.5 + 0.4 * torch.tanh(torch.randn(n, generator=g))
    kept = []
    for b, c in enumerate(sizes):
        lo = int(ptr[b])
        if c == 0:
            continue
        if chain and b == len(sizes) - 1:
            kept.append(torch.tensor([lo]))
            continue
        k = {"one": 1, "half": -(-c // 2), "all": c}[cfg["keep"]]
        kept.append(torch.randperm(c, generator=g)[:k].sort().values + lo)
    d["kept"] = torch.cat(kept)
    d["wgrad_rows"] = [int(limits["maxcut_wgrad_rows"]) + k for k in (-1, 0, 1)] + [2 * int(limits["maxcut_wgrad_rows"]) + 1]
    return d


def gtv_margins(h, edge_index, edge_weight, bias, mask, delta, eps, act):
    """How far the propagation's kinks stay from float64 rows ``h``: (the smallest nonzero channel difference |h_ic -
    h_jc| over the non-loop edges, the smallest |d_e - eps| / eps, for relu the smallest |pre-activation| over the rows
    the mask keeps -- a masked row is an exact zero with slope x mask = 0 on both sides -- and inf otherwise)."""
    import gtv_restatement as R
    inf = float("inf")
    diff, dist = R.distances(h, edge_index)
    pos = diff[diff > 0]
    gap = float(pos.min()) if pos.numel() else inf
    near = float(((dist - eps).abs() / eps).min()) if dist.numel() else inf
    pre = inf
    if act == "relu":
        z = R.propagate(h, edge_index, None if edge_weight is None else edge_weight.to(h.dtype),
                        None if bias is None else bias.to(h.dtype), None, delta, eps, None)
        z = z if mask is None else z[mask]
        pre = float(z.abs().min()) if z.numel() else inf
    return gap, near, pre


def gtv_draw_margins(d):
    """The three margins of a draw, the worse of its two layers: the operator layer's rows ``h`` (with the mask) and the
    public layer's ``x @ weight`` (sparse mode takes no mask), both in float64."""
    op = gtv_margins(d["h"].double(), d["edge_index"], d["edge_weight"], d["bias"], d["mask"], d["delta"], d["eps"], d["act"])
    pub = gtv_margins(d["x"].double() @ d["weight"].double(), d["edge_index"], d["edge_weight"], d["bias"], None,
                      d["delta"], d["eps"], d["act"])
    return tuple(min(a, b) for a, b in zip(op, pub))


def _gtv_candidate(cfg, g):
    sizes, C = cfg["sizes"], cfg["C"]
    d = dict(cfg)
    ptr = _ptr(sizes)
    n = int(ptr[-1])
    parts = [_edges(c, min(0.3, 4.0 / max(c, 1)), cfg["directed"], g, self_loops=cfg["dups_loops"],
                    duplicates=cfg["dups_loops"]) + int(ptr[i]) for i, c in enumerate(sizes)]
    ei = torch.cat(parts, 1)
    # the two hubs sit in the longest graph (at least 3 nodes): v takes in-edges only from, u sends out-edges only to,
    # the nodes that are neither (repeats: duplicates), so that both degrees are exact
    big = max(range(len(sizes)), key=lambda i: sizes[i])
    lo, c = int(ptr[big]), sizes[big]
    v, u = lo, lo + c // 2
    rest = torch.tensor([i for i in range(lo, lo + c) if i not in (u, v)])
    ei = ei[:, (ei[0] != u) & (ei[0] != v) & (ei[1] != v)]
    pick = lambda k: rest[torch.randint(0, rest.numel(), (k,), generator=g)]  # noqa: E731
    src, dst = pick(cfg["in_hub"]), pick(cfg["out_hub"])
    ei = torch.cat([ei, torch.stack([src, torch.full_like(src, v)]), torch.stack([torch.full_like(dst, u), dst]),
                    torch.stack([torch.tensor([v]), pick(1)])], 1)
    if cfg["dups_loops"]:  # (skipped by the kernels: neither hub's degree counts them)
        ei = torch.cat([ei, torch.tensor([[u, v], [u, v]])], 1)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    if cfg["order"] != "shuffled":
        ei = ei[:, torch.argsort(ei[1 if cfg["order"] == "by_destination" else 0], stable=True)]
    ei = ei.contiguous()
    E = ei.size(1)
    ew = None
    if cfg["weighted"]:
        ew = torch.rand(E, generator=g) + 0.25
        ew[torch.rand(E, generator=g) < 0.1] = 0.0
    # rows: N(0, 1); three joined pairs are made twins -- h_j = h_i except in at most two channels, which differ by
    # 0.05 .. 0.12 (d_e in 0.05 .. 0.24: clamped at eps = 0.5, free at 1e-3; every other channel difference an exact 0)
    # -- and under eps = 0.5 one pair is equal in every channel (d_e = 0; at eps = 1e-3 its gamma of 1000 w would
    # drown every other term of dh)
    h = torch.randn(n, C, generator=g)
    x = torch.randn(n, GTV_F_IN, generator=g)
    real = (ei[0] != ei[1]).nonzero().view(-1)
    twins, used = [], set()
    for e in real[torch.randperm(real.numel(), generator=g)].tolist():  # (pairs that share no node: none undoes another)
        if len(twins) < 4 and not {int(ei[0, e]), int(ei[1, e])} & used:
            twins.append(e)
            used |= {int(ei[0, e]), int(ei[1, e])}
    for k, e in enumerate(twins):
        i, j = int(ei[0, e]), int(ei[1, e])
        h[j] = h[i]
        if k == 0 and cfg["eps"] == 0.5:
            x[j] = x[i]
            continue
        ch = torch.randperm(C, generator=g)[:2]
        step = 0.05 + 0.07 * torch.rand(ch.numel(), generator=g)
        h[j, ch] += torch.where(torch.rand(ch.numel(), generator=g) < 0.5, -step, step)
    d.update(edge_index=ei, edge_weight=ew, ptr=ptr, n=n, batch=_batch(sizes), h=h, x=x, twin_edges=twins,
             weight=torch.randn(GTV_F_IN, C, generator=g) * (2.0 / GTV_F_IN) ** 0.5,
             bias=torch.randn(C, generator=g) * 0.3 if cfg["bias"] else None,
             mask=(torch.rand(n, generator=g) < 0.7) if cfg["mask"] else None, out_hub_node=u, in_hub_node=v)
    d["form"] = gtv_load_form(C, cfg["layout"])
    return d


def _draw_gtv(cfg, g, limits):
    """h [n, C] (the operator layer's rows), x [n, 5] and weight [5, C] (the public layer's: h = x @ weight), the list in
    the drawn order with the two hubs, weights (a tenth exact zeros) or None, bias or None, a node mask or None.

    The propagation has kinks: |h_ic - h_jc| at 0, max(d_e, eps) at d_e = eps, relu at 0.  A float32 product on the other
    side of one differs from the float64 reference by a whole term, not by rounding, so -- the separation rule of
    ``GradCase`` in tests/test_gpu_gtv.py -- sub-seeds are walked until, in float64 and for both layers, no edge has a
    channel difference in (0, GTV_MARGIN), no distance lies within GTV_MARGIN eps of eps and, for relu, no pre-activation
    of a kept row lies within GTV_MARGIN of 0.  No draw is given up: 200 sub-seeds that all fail raise."""
    base = int(g.initial_seed())
    for sub in range(GTV_SUB_SEEDS):
        d = _gtv_candidate(cfg, torch.Generator().manual_seed(base * 1009 + sub))
        gap, near, pre = gtv_draw_margins(d)
        if gap >= GTV_MARGIN and near >= GTV_MARGIN and pre >= GTV_MARGIN:
            d["sub_seed"] = sub
            return d
    raise RuntimeError(f"gtv seed {cfg['seed']}: {GTV_SUB_SEEDS} sub-seeds did not keep the kinks away")


def pan_cut_gap(score, batch, sizes, ratio=0.5):
    """The smallest distance between a kept and a dropped score over the graphs (top ceil(ratio n_b) of each): inf where
    every node of every graph is kept."""
    gap, lo = float("inf"), 0
    for c in sizes:
        k = -(-c * ratio // 1)
        s = torch.sort(score[lo:lo + c], descending=True).values
        if 0 < k < c:
            gap = min(gap, float(s[int(k) - 1] - s[int(k)]))
        lo += c
    return gap


def _draw_pan(cfg, g, limits):
    """The list of a sorted batch (random endpoints: loops and multi-edges as they fall; mirrored unless directed; graphs
    above 200 nodes at a mean degree of 1.5) plus one more graph, the hub: ``hub`` nodes that all reach its first node
    within min(filter_size, 2) hops, so that this row of M stores exactly ``hub`` entries.  ``weight`` [L + 1] with |w|
    in [0.4, 0.9], one exact zero or one negative entry where drawn (the pattern is structural: it must not change).
    The public layer's x, ``lin``, ``p`` and ``beta`` are walked over sub-seeds until the float64 scores of every graph
    keep PAN_GAP between the kept and the dropped nodes (the selection is a top-k: the kept SET is compared exactly).
    The scorer's own inputs: x [n, score_F], p, beta, and a list of entries with values in which one node's column group
    holds exactly ``score_group`` entries."""
    import pan_restatement as R
    d = dict(cfg)
    L, k = cfg["filter_size"], cfg["hub"]
    sizes = list(cfg["sizes"]) + [k]
    ptr = _ptr(sizes)
    n = int(ptr[-1])
    parts = []
    for i, c in enumerate(cfg["sizes"]):
        m = int(c * (1.5 if c > 200 else (0.5, 1.5, 3.0)[i % 3])) if c > 1 else 0
        e = torch.randint(0, c, (2, m), generator=g)
        parts.append((e if cfg["directed"] else torch.cat([e, e.flip(0)], 1)) + int(ptr[i]))
    direct = max(1, (k - 1) // 2) if L >= 2 else k - 1  # the hub: nodes 1 .. direct point at node 0, the rest at one of them
    src = torch.arange(1, k)
    dst = torch.where(src <= direct, torch.zeros_like(src), 1 + torch.randint(0, max(direct, 1), (k - 1,), generator=g))
    parts.append(torch.stack([src, dst]) + int(ptr[-2]))
    ei = torch.cat(parts, 1)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    if cfg["order"] == "by_source":
        ei = ei[:, torch.argsort(ei[0], stable=True)]
    w = 0.4 + 0.5 * torch.rand(L + 1, generator=g)
    at = int(torch.randint(1, L + 1, (1,), generator=g)) if L > 0 else 0
    if cfg["weights"] == "zero":
        w[at] = 0.0
    elif cfg["weights"] == "negative":
        w[at] = -w[at]
    batch = _batch(sizes)
    d.update(all_sizes=sizes, ptr=ptr, n=n, batch=batch, edge_index=ei.contiguous(), weight=w, hub_row=int(ptr[-2]),
             route="native" if max(sizes) <= int(limits["pan_max_graph_nodes"]) else "composed")
    # the scorer's own inputs
    f, t = cfg["score_F"], n // 2
    idx = torch.randint(0, n, (2, 3 * n), generator=g)
    idx = torch.cat([idx[:, idx[1] != t], torch.stack([torch.randint(0, n, (cfg["score_group"],), generator=g),
                                                       torch.full((cfg["score_group"],), t)])], 1)
    idx = idx[:, torch.argsort(idx[0] * n + idx[1], stable=True)].contiguous()
    d.update(score_index=idx, score_values=torch.randn(idx.size(1), generator=g), score_node=t,
             score_x=torch.randn(n, f, generator=g), score_p=torch.randn(f, generator=g) / f ** 0.5,
             beta=torch.tensor([0.7, -1.3]))
    index, values = R.met(d["edge_index"], w.double(), n, batch)
    base = int(g.initial_seed())
    for sub in range(PAN_SUB_SEEDS):
        gen = torch.Generator().manual_seed(base * 1013 + sub)
        x = torch.randn(n, PAN_F, generator=gen)
        lin_w, lin_b = torch.randn(PAN_F, PAN_F, generator=gen) * 0.5, torch.randn(PAN_F, generator=gen) * 0.1
        p = torch.randn(PAN_F, generator=gen)
        p = p / p.norm()
        h = torch.zeros(n, PAN_F, dtype=torch.float64).index_add(0, index[0], values.view(-1, 1) * x.double()[index[1]])
        h = h @ lin_w.double().t() + lin_b.double()
        score = torch.tanh(R.raw_score(h, index, values, p.double(), d["beta"].double()))
        if pan_cut_gap(score, batch, sizes) >= PAN_GAP:
            d.update(x=x, lin_w=lin_w, lin_b=lin_b, p=p, sub_seed=sub)
            return d
    raise RuntimeError(f"pan seed {cfg['seed']}: {PAN_SUB_SEEDS} sub-seeds left no gap at the cut")


def _draw_eigenpool(cfg, g, limits):
    """Modes and the public layer: two graphs of EIG_K clusters, the nodes of a graph's clusters interleaved (``labels``),
    one cluster of the first graph empty; every group connected (a path through it) and dense (half of its pairs), with
    distinct weights in [0.1, 1) that separate its spectrum; as many weighted edges between a graph's clusters again;
    the list symmetric and shuffled; x [n, 3].  Reduce and Lift on inputs of their own: groups of ``rows`` rows (the
    longest among short ones, which leave most of the 4 or 16 waves without a row) interleaved in node order, any
    values for theta [rows, reduce_H], x [rows, F] and x_pool [G, reduce_H F]."""
    d = dict(cfg)
    sizes, k = cfg["sizes"], EIG_K
    ptr = _ptr(sizes)
    n = int(ptr[-1])
    labels = torch.cat([torch.repeat_interleave(torch.arange(k), torch.tensor(c))[torch.randperm(sum(c), generator=g)]
                        for c in cfg["clusters"]])
    batch = _batch(sizes)
    gid = batch * k + labels
    a = torch.zeros(n, n)
    for grp in gid.unique().tolist():
        nodes = (gid == grp).nonzero().view(-1)
        m = nodes.numel()
        up = torch.triu(torch.rand(m, m, generator=g) < 0.5, 1)
        if m > 1:
            up |= torch.diag(torch.ones(m - 1, dtype=torch.bool), 1)
        w = torch.triu(torch.rand(m, m, generator=g) * 0.9 + 0.1, 1) * up
        a[nodes.view(-1, 1), nodes.view(1, -1)] = w + w.t()
    across = (batch.view(-1, 1) == batch.view(1, -1)) & (gid.view(-1, 1) != gid.view(1, -1))
    w = torch.triu((torch.rand(n, n, generator=g) < 4.0 / n) * (torch.rand(n, n, generator=g) * 0.9 + 0.1), 1) * across
    a = a + w + w.t()
    ei = a.nonzero().t()
    order = torch.randperm(ei.size(1), generator=g)
    ei = ei[:, order].contiguous()
    d.update(n=n, ptr=ptr, batch=batch, labels=labels, gid=gid, edge_index=ei, edge_weight=a[ei[0], ei[1]].contiguous(),
             x=torch.randn(n, 3, generator=g), width=k)
    rows = cfg["rows"]
    total, G = sum(rows), len(rows)
    rgid = _batch(rows)[torch.randperm(total, generator=g)]
    d.update(reduce_gid=rgid, reduce_groups=G, theta=torch.randn(total, cfg["reduce_H"], generator=g),
             reduce_x=torch.randn(total, cfg["F"], generator=g),
             reduce_y=torch.randn(G, cfg["reduce_H"] * cfg["F"], generator=g))
    return d


_DRAW = {"gtv": _draw_gtv, "pan": _draw_pan, "eigenpool": _draw_eigenpool, "asap": _draw_asap, "maxcut": _draw_maxcut, "jb": _draw_jb, "dmon": _draw_dmon, "hosc": _draw_dmon, "acc": _draw_acc, "bnpool": _draw_bnpool,
         "lapool": _draw_lapool, "readout": _draw_readout, "sag": _draw_sag, "kmis": _draw_selector,
         "edge_contract": _draw_selector}


def draw(family, seed, limits):
    """The inputs of (family, seed): CPU tensors plus the configuration they were drawn from."""
    cfg = plan(family, limits)[seed]
    return _DRAW[family](cfg, _gen(family, seed), limits)


def library_limits():
    """The limits the draws straddle, read from the library's own queries (host calls: no device is touched)."""
    from tgp import kernels as K
    lib = K.N.lib()
    width = int(K.maxcut_max_width())
    bytes_at = lambda n: int(lib.tgp_maxcut_wgrad_workspace_bytes(n, width, width))  # noqa: E731
    lo, hi = 1, 2
    while bytes_at(hi) == bytes_at(1):  # the rows of one partial sum: the last n before the workspace takes its first step
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if bytes_at(mid) == bytes_at(1) else (lo, mid)
    return {"maxcut_wgrad_rows": lo, "maxcut_max_width": width, "part_rows": int(K._PART_ROWS), "segment_chunk_rows": int(K.segment_aggr_chunk_rows()),
            "kmis_max_graph_nodes": int(lib.tgp_kmis_max_graph_nodes()),
            "edge_contract_max_graph_nodes": int(lib.tgp_edge_contract_max_graph_nodes()),
            "bnpool_max_clusters": int(K.bnpool_max_clusters()),
            "hosc_small_graph_nodes": int(K.hosc_small_graph_nodes()),
            "acc_small_graph_nodes": int(K.acc_small_graph_nodes()), "acc_tv_rows": int(K._ACC_TV_ROWS),
            "gtv_register_channels": int(K.GTV_REGISTER_CHANNELS), "pan_max_graph_nodes": int(K.pan_max_graph_nodes()),
            "eigenpool_max_group_nodes": int(K.eigenpool_max_group_nodes())}
