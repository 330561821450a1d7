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
MaxCut's score net, cut loss and assignment rounds ("maxcut").  New families are APPENDED: ``_gen`` seeds from a
family's position in ``FAMILIES``.
"""
import random

import torch

FAMILIES = ("jb", "readout", "sag", "kmis", "edge_contract", "bnpool", "dmon", "hosc", "acc", "lapool", "asap", "maxcut")
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
}
# limits a draw reads without drawing graph sizes around them (the rows per partial sum of MaxCut's weight gradient,
# the widest row its kernels take)
DRAW_LIMITS = {"maxcut": ("maxcut_wgrad_rows", "maxcut_max_width")}
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


def _plan(family, limits, rng):
    n = len(SEEDS)
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


_DRAW = {"asap": _draw_asap, "maxcut": _draw_maxcut, "jb": _draw_jb, "dmon": _draw_dmon, "hosc": _draw_dmon, "acc": _draw_acc, "bnpool": _draw_bnpool,
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
            "acc_small_graph_nodes": int(K.acc_small_graph_nodes()), "acc_tv_rows": int(K._ACC_TV_ROWS)}
