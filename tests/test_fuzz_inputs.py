"""The generator and the comparison rule of the family sweep, on the CPU (tests/fuzz_inputs.py, tests/fuzz_compare.py).

* ``draw`` is deterministic, and over a family's 16 seeds every listed boundary value, layout and route class is drawn:
  asserted against the generator's own lists, so a thinned generator fails.
* Every index is in range, every ``ptr`` monotone, every edge inside its graph.
* Conditioning: the float32 restatement against the float64 one stays within CAP / FACTOR on every (family, seed), for
  the values and (through ``grad_path_errors``, which holds the cap itself) for the gradients.
* The harness finds faults: with the float32 restatement standing in for the kernels every seed passes; wrong Python
  stand-ins (a dropped row, ties resolved the wrong way, a scaled term; for ASAP an arg-max tie resolved to the higher
  edge position and an edge softmax that loses a group's 65th edge, for MaxCut a diagonal term above n_P) are each
  flagged on at least one seed, by the name of the output.
"""
import pytest
import torch

import fuzz_inputs as FI
import fuzz_refs as FR
from fuzz_compare import CAP, FACTOR, conditioning, forward_errors, grad_path_errors

_LIMITS = {}


def limits():
    """The library's limits, read on first use: a tree without the built library fails its tests, not the collection."""
    if not _LIMITS:
        _LIMITS.update(FI.library_limits())
    return _LIMITS


def _dmon_raw(d):
    return d["s"].transpose(1, 2) @ d["adj"] @ d["s"]


FLOAT_REFS = {"jb": FR.jb_reference, "readout": FR.readout_reference, "sag": FR.sag_reference,
              "bnpool": FR.bnpool_reference, "bnpool_operators": FR.bnpool_operator_reference,
              "dmon": lambda d, dt: FR.dmon_reference(d, dt, _dmon_raw(d), grads=True),
              "acc": FR.acc_reference,
              "lapool": lambda d, dt: FR.lapool_reference(d, dt, FR.lapool_leaders(d, FR.lapool_variation(d, torch.float32))),
              "acc_flat": lambda d, dt: FR.acc_flat_reference(d, dt) if d["prefix"] else ({}, {}),
              "hosc": lambda d, dt: FR.hosc_reference(d, dt, _dmon_raw(d) if d["with_raw"] else None, grads=True),
              "asap": FR.asap_reference, "asap_operators": FR.asap_operator_reference,
              "maxcut": FR.maxcut_reference, "maxcut_operators": FR.maxcut_operator_reference}
ASAP_PARAMS = ["lin.weight", "lin.bias", "att.weight", "att.bias", "select_scorer.lin1.weight", "select_scorer.lin1.bias",
               "select_scorer.lin2.weight", "select_scorer.lin3.weight", "select_scorer.lin3.bias"]
# (every name a drawn score net can have: 1 ... 4 layers, a tail of up to two Linear; a leaf a draw lacks is skipped)
MAXCUT_PARAMS = [FR.RM.PRE + n + e for n in ["initial_layer", "final_layer", "mlp.0", "mlp.1"] for e in (".weight", ".bias")] \
    + [f"{FR.RM.PRE}mp_convs.{l}{e}" for l in range(4) for e in (".lin.weight", ".bias")]
LEAVES = {"jb": ["s"], "readout": ["x", "weight"], "sag": ["x", "w_rel", "w_root", "b"], "bnpool": ["s", "k_mat"],
          "bnpool_operators": ["t", "s"], "dmon": ["s", "raw"], "hosc": ["s", "raw"], "acc": ["s"],
          "acc_flat": ["s"], "lapool": ["x"], "asap": ["x", "x_pool"] + ASAP_PARAMS,
          "asap_operators": ["x", "x_pool", "sq_in", "sp_in", "val", "p"], "maxcut": ["x", "s"] + MAXCUT_PARAMS,
          "maxcut_operators": ["z0", "z1", "z2", "z3", "h_tail", "s"]}


def draws(family):
    return [FI.draw(family, s, limits()) for s in FI.SEEDS]


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):  # (a draw's parameters by name)
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return a == b


@pytest.mark.parametrize("family", FI.FAMILIES)
def test_draw_is_deterministic(family):
    first = draws(family)
    FI._PLANS.clear()
    for a, b in zip(first, draws(family)):
        assert set(a) == set(b)
        for k in a:
            assert _same(a[k], b[k]), (family, a["seed"], k)


@pytest.mark.parametrize("family", FI.FAMILIES)
def test_every_boundary_value_layout_and_route_is_drawn(family):
    ds = draws(family)
    assert {v for d in ds for v in d["sizes"]} >= set(FI.row_values(family, limits()))
    for name in FI.LIMITS[family]:
        lim = limits()[name]
        assert {lim - 1, lim, lim + 1} <= {v for d in ds for v in d["sizes"]}
    assert {d["B"] for d in ds} == set(FI.BATCHES) and all(len(d["sizes"]) == d["B"] for d in ds)
    assert {d["layout"] for d in ds} == set(FI.LAYOUTS[family])
    for d in ds:
        if d["B"] >= 3:  # a graph of 0 rows, and (N = the longest graph) one that fills the padded size
            assert 0 in d["sizes"] and max(d["sizes"]) > 0
        assert sum(d["sizes"]) > 0
    assert any(0 < d["sizes"].index(0) < d["B"] - 1 for d in ds if 0 in d["sizes"])  # an empty id in the middle
    if family == "jb":
        assert {d["K"] for d in ds} == set(FI.CLUSTERS)
        assert any(d["zero_col"] for d in ds) and any(not d["zero_col"] for d in ds)
        part = limits()["part_rows"]
        assert {max(d["sizes"]) > part for d in ds} == {True, False}  # one launch / the partial pass and a tail
        assert any(0 in d["n_b"] for d in ds)  # a graph without a real node
    if family == "lapool":
        assert {d["F"] for d in ds} == set(FI.FEATURES) and {d["density"] for d in ds} == set(FI.DENSITIES)
        assert {d["directed"] for d in ds} == {True, False} and {d["weighted"] for d in ds} == {True, False}
        assert any(not d["padded"] and d["edge_weight"] is not None and bool((d["edge_weight"] == 0).any()) for d in ds)
        assert any(not d["padded"] and bool((d["edge_index"][0] == d["edge_index"][1]).any()) for d in ds)  # self-loops
        for d in ds:  # tied variations: the leader rule is decided on equal values somewhere
            assert d["v_tied"].unique().numel() <= 4
    if family == "acc":
        small, tv_rows = limits()["acc_small_graph_nodes"], limits()["acc_tv_rows"]
        assert {d["loss_k"] for d in ds} == {1, 2, 3, 7} and {d["ties"] for d in ds} == {True, False}
        assert {d["N"] <= small for d in ds} == {True, False}  # the counting select / the radix select
        assert {tv_rows - 1, tv_rows, tv_rows + 1, 31, 32, 33} <= {v for d in ds for v in d["sizes"]}
        assert any(64 < d["in_degree_max"] <= 256 for d in ds) and any(d["in_degree_max"] > 256 for d in ds)
        assert {d["edge_weight"] is None for d in ds if d["prefix"]} == {True, False}
        tied = 0
        for d in ds:  # where ties are drawn the quantile value really is held by several rows of some column
            if d["ties"] and d["loss_k"] > 1:
                a, b = FR.acc_quantile_exact(d)["qnode"], FR.acc_quantile_exact(d, higher=True)["qnode"]
                tied += int((a != b).sum())
        assert tied > 0
    if family == "hosc":
        small = limits()["hosc_small_graph_nodes"]
        assert {d["alpha"] for d in ds} == {0.0, 0.5, 1.0} and {d["hosc_ortho"] for d in ds} == {True, False}
        assert {d["with_raw"] for d in ds} == {True, False}
        routes = {(d["N"] <= small and d["K"] <= small) for d in ds if d["alpha"] > 0}
        assert routes == {True, False}  # the one-launch forward and the general route, both with the motif term on
        assert any(d["N"] == small and d["K"] <= small and d["alpha"] > 0 for d in ds)
    if family in ("dmon", "hosc", "acc"):
        assert {d["K"] for d in ds} == set(FI.CLUSTERS) and {d["density"] for d in ds} == set(FI.DENSITIES)
        assert {d["directed"] for d in ds} == {True, False} and {d["weighted"] for d in ds} == {True, False}
        part = limits()["part_rows"]
        assert {d["N"] > part for d in ds} == {True, False} and any(0 in d["n_b"] for d in ds)
        assert any(d["prefix"] and max(d["n_b"]) > part for d in ds)  # the un-padded partial pass with more than a block
        for d in ds:  # the values of the spectral term are compared too: not only on draws without an edge
            assert float(d["adj"].sum()) > 0 or d["density"] < 0.2 or d["N"] < 3
    if family == "bnpool":
        kmax = limits()["bnpool_max_clusters"]
        assert {d["K"] for d in ds} == set(FI.CLUSTERS) | {kmax, kmax // 2}
        assert {d["density"] for d in ds} == set(FI.DENSITIES)
        assert {d["directed"] for d in ds} == {True, False} and {d["weighted"] for d in ds} == {True, False}
        assert any(0 in d["n_b"] for d in ds)
        assert {31, 32, 33} <= {d["N"] for d in ds} | {v for d in ds for v in d["sizes"]}  # around the 32 x 32 tile
    if family == "readout":
        assert {d["F"] for d in ds} == set(FI.FEATURES)
        assert {d["ops"] for d in ds} == set(FI.READOUT_SUBSETS) and len(FI.READOUT_SUBSETS) == 15
        assert {d["integer"] for d in ds} == {True, False}
        assert {d["max_len"] > limits()["segment_chunk_rows"] for d in ds} == {True, False}  # one chain / the split route
    if family == "sag":
        assert {d["F"] for d in ds} == set(FI.FEATURES)
        assert {d["density"] for d in ds} == set(FI.DENSITIES)
        assert {d["directed"] for d in ds} == {True, False} and {d["mean"] for d in ds} == {True, False}
        assert {d["order"] for d in ds} == {"sorted", "shuffled"}
        assert {d["root"] for d in ds} == {True, False} and {d["bias"] for d in ds} == {True, False}
        assert any(64 < d["in_degree_max"] <= 256 for d in ds) and any(d["in_degree_max"] > 256 for d in ds)
    if family in ("asap", "maxcut"):
        assert {d["density"] for d in ds} == set(FI.DENSITIES) and {d["order"] for d in ds} == set(FI.EDGE_ORDERS)
        assert {d["directed"] for d in ds} == {True, False} and {d["weighted"] for d in ds} == {True, False}
        assert {d["hub"] for d in ds} == set(FI.EDGE_HUBS)
        for d in ds:  # the hub is there: one node of the list has at least that many in-edges, exactly that many at 63 ... 65
            indeg = torch.bincount(d["edge_index"][1], minlength=d["n"])
            assert d["hub"] == 0 or d["hub"] in indeg.tolist(), (d["seed"], d["hub"])
        # both index forms in both directions: offsets only (perm None) and a permutation, on lists that have edges
        forms = {(by_dst, FR.edge_group_exact(d["edge_index"], d["n"], by_dst)["perm"] is None)
                 for d in ds if d["edge_index"].size(1) > 1 for by_dst in (True, False)}
        assert forms == {(True, True), (True, False), (False, True), (False, False)}
        assert any(d["edge_weight"] is not None and bool((d["edge_weight"] == 0).any()) for d in ds)  # explicit zeros
        assert any(bool((d["edge_index"][0] == d["edge_index"][1]).any()) for d in ds)  # self-loops
        assert any(torch.unique(d["edge_index"], dim=1).size(1) < d["edge_index"].size(1) for d in ds)  # duplicates
        sizes = lambda d: d.get("all_sizes", d["sizes"])  # noqa: E731
        # a graph of 0 and of 1 nodes inside a batch; node ranges without an edge at the start and at the end of a batch;
        # a list that does not reach N in a batch of several graphs
        assert any(0 in sizes(d) and d["B"] > 1 for d in ds) and any(1 in sizes(d) and d["B"] > 1 for d in ds)
        touched = [torch.bincount(d["edge_index"].reshape(-1), minlength=d["n"]) > 0 for d in ds]
        assert any(t.any() and not t[0] for t in touched) and any(t.any() and not t[-1] for t in touched)
        assert any(d["B"] > 1 and d["edge_index"].numel() and int(d["edge_index"].max()) + 1 < d["n"] for d in ds)
    if family == "asap":
        from tgp import kernels as K
        assert set(FI.ASAP_ACT_NAMES) == set(K.ASAP_ACTS) and {d["act"] for d in ds} == set(FI.ASAP_ACT_NAMES)
        assert sorted(d["F"] for d in ds) == sorted(FI.ASAP_FEATURES) and len(FI.ASAP_FEATURES) == len(FI.SEEDS)
        for d in ds:  # the form and the lane count are the rule's, from F, stride and pointer
            stride, first = FI.asap_row_geometry(d["F"], d["layout"])
            vec = d["F"] >= 4 and stride % 4 == 0 and first % 16 == 0
            assert d["form"] == ("vec16" if vec else "scalar")
            units = -(-d["F"] // 4) if vec else d["F"]
            assert d["lanes"] == min([g for g in FI.ASAP_LANES[d["form"]] if g >= units], default=64)
        assert {d["form"] for d in ds} == {"vec16", "scalar"}
        # (on draws whose list has edges in groups of several: a kernel that walks no edge shows nothing)
        walked = [d for d in ds if d["in_degree_max"] > 2]
        vec = {d["F"]: d["lanes"] for d in walked if d["form"] == "vec16"}
        assert set(vec.values()) == set(FI.ASAP_LANES["vec16"])  # every G of the 16-byte form, 4 and 8 among them
        assert 8 in vec and {12, 16} & set(vec) and 32 in vec and {257, 260} & set(vec)  # (257, 260: the second block)
        assert {d["form"] for d in walked if d["F"] == 260} == {"scalar"}
        assert {d["lanes"] for d in walked if d["form"] == "scalar"} == set(FI.ASAP_LANES["scalar"])
        assert {d["negative_slope"] for d in ds} == {0.2, 0.0} and {d["bias"] for d in ds} == {True, False}
        assert {d["same_pool"] for d in ds} == {True, False}
        assert all((d["x_pool"] is d["x"]) == d["same_pool"] for d in ds)
        assert {d["alpha_mask"] is not None for d in ds} == {True, False}
        assert any(d["alpha_mask"] is not None and 0 < int((d["alpha_mask"] == 0).sum()) < d["alpha_mask"].numel() for d in ds)
        tied = [d for d in ds if d["x_tied"] is not None]
        assert tied and any(FR.asap_tied_sources(dict(d, x_pool=d["x_tied"])) > 0 for d in tied)
    if family == "maxcut":
        from tgp import kernels as K
        assert set(FI.MAXCUT_ACT_NAMES) == set(K.MAXCUT_ACTS)
        for name in ("mp_act", "mlp_act", "act"):
            assert {d[name] for d in ds} == set(FI.MAXCUT_ACT_NAMES)
        assert {w for d in ds for w in d["widths"]} == set(FI.MAXCUT_WIDTHS) and {d["F"] for d in ds} == set(FI.MAXCUT_WIDTHS[1:])
        assert {len(d["widths"]) for d in ds} == {1, 2, 3, 4}
        pairs = [(a, b) for d in ds for a, b in zip(d["widths"][:-1], d["widths"][1:])]
        assert all(a != b for a, b in pairs)
        cross = lambda a, b: FI.pow2_ceil(a) != FI.pow2_ceil(b)  # noqa: E731  (another lane count per row)
        assert any(b > a and cross(a, b) for a, b in pairs) and any(b < a and cross(a, b) for a, b in pairs)
        assert {d["delta"] for d in ds} == {0.5, 2.0} and {d["tail"] for d in ds} == set(FI.MAXCUT_TAILS)
        wmax = limits()["maxcut_max_width"]
        for d in ds:  # the tail that does not fit is wider than the widest row; every other tail is within it
            assert (max(d["mlp_units"], default=0) > wmax) == (d["tail"] == "unfit")
        assert {d["np_class"] for d in ds} == set(FI.NP_CLASSES)
        for d in ds:
            ei = d["edge_index"]
            assert d["n_p"] == (int(ei.max()) + 1 if ei.numel() else 0)
            assert {"full": d["n_p"] == d["n"], "below": 0 < d["n_p"] < d["n"] or d["n"] <= 2, "empty": ei.numel() == 0,
                    "loops": ei.numel() > 0 and bool((ei[0] == ei[1]).all())}[d["np_class"]], (d["seed"], d["np_class"])
            assert d["edge_weight"] is None or bool((d["edge_weight"] >= 0).all())
        assert any(d["np_class"] == "below" and d["B"] > 1 and d["n_p"] < d["n"] for d in ds)
        zero = [d for d in ds if d["zero_degree_node"] is not None]
        assert zero  # a node with out-edges to other nodes whose degree is 0: dinv goes inf -> 0
        for d in zero:
            out = (d["edge_index"][0] == d["zero_degree_node"]) & (d["edge_index"][1] != d["zero_degree_node"])
            assert bool(out.any()) and float(d["edge_weight"][out].sum()) == 0.0
            assert float(FR.RM.dinv_of(d["edge_index"], d["edge_weight"], d["n"])[d["zero_degree_node"]]) == 0.0
        assert {d["keep"] for d in ds} == set(FI.MAXCUT_KEEP) and {d["max_iter"] for d in ds} == {1, 5}
        for d in ds:  # between 1 and all nodes of every graph with a node are kept
            per = torch.bincount(d["batch"][d["kept"]], minlength=len(d["all_sizes"]))
            assert all((0 < k <= c) if c else k == 0 for k, c in zip(per.tolist(), d["all_sizes"]))
            assert bool((d["kept"][1:] > d["kept"][:-1]).all())
        chains = [d for d in ds if d["chain"]]
        assert chains
        for d in chains:  # the path's tail is still unlabelled after max_iter rounds, and one more round would go on
            label = FR.maxcut_labels_exact(d)
            assert int(label[-1]) == 0 and int(label[d["n"] - d["all_sizes"][-1] + d["max_iter"]]) > 0
        L = limits()["maxcut_wgrad_rows"]
        assert all(d["wgrad_rows"] == [L - 1, L, L + 1, 2 * L + 1] for d in ds)
    if family in ("kmis", "edge_contract"):
        assert {d["density"] for d in ds} == set(FI.DENSITIES) and {d["directed"] for d in ds} == {True, False}
        assert {d["route"] for d in ds} == {"graphs", "rounds"}
        big = [d for d in ds if d["big"]]
        assert big and all(d["big_entries"] > FI.FRAME_CACHE_ENTRIES and 600 in d["all_sizes"] for d in big)
        assert any(d["route"] == "graphs" for d in big)  # the LDS edge cache overflows on the per-graph route
        lim = limits()[FI.LIMITS[family][0]]
        assert any(d["route"] == "graphs" and max(d["all_sizes"]) == lim for d in ds)  # the limit itself still fits
        if family == "kmis":
            assert {d["order_k"] for d in ds} == set(FI.ORDER_K)
        for d in ds:  # tied scores: the order is decided by the rule for ties
            assert d["score"].numel() == 0 or d["score"].unique().numel() < max(d["score"].numel(), 2)


@pytest.mark.parametrize("family", FI.FAMILIES)
def test_every_index_is_in_range(family):
    for d in draws(family):
        for name in ("ptr", "graph_ptr", "edge_ptr"):
            p = d.get(name)
            if p is not None:
                assert int(p[0]) == 0 and bool((p[1:] >= p[:-1]).all())
        if "edge_index" in d:
            ei, n = d["edge_index"], d["n"]
            assert ei.dtype == torch.long and (ei.numel() == 0 or (0 <= int(ei.min()) and int(ei.max()) < n))
            sizes = d.get("all_sizes", d["sizes"])
            owner = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
            if family != "sag" or not d["hub"]:  # (the scorer's hub collects sources from the whole batch)
                assert torch.equal(owner[ei[0]], owner[ei[1]])
            if d.get("graph_ptr") is not None:
                assert bool((ei[0, 1:] >= ei[0, :-1]).all()) and int(d["graph_ptr"][-1]) == n
                assert d["max_graph_nodes"] == max(sizes)
            assert sorted(d["perm"].tolist()) == list(range(d["perm"].numel())) if "perm" in d else True
        if family == "readout":
            rows = d["x"].reshape(-1, d["F"]).size(0)
            assert d["src_rows"].numel() == d["index"].numel()
            assert d["index"].numel() == 0 or (0 <= int(d["index"].min()) and int(d["index"].max()) < d["groups"])
            assert d["src_rows"].numel() == 0 or (0 <= int(d["src_rows"].min()) and int(d["src_rows"].max()) < rows)
            assert int(torch.bincount(d["index"], minlength=1).max()) <= d["max_len"]
        if family == "jb" and not d["padded"]:
            assert d["s"].size(0) == int(d["ptr"][-1]) == d["batch"].numel()
        if family in ("asap", "maxcut"):
            assert d["x"].shape == (d["n"], d["F"]) and d["batch"].numel() == d["n"] == int(d["ptr"][-1])
            assert d["edge_weight"] is None or d["edge_weight"].shape == (d["edge_index"].size(1),)
        if family == "asap":
            # no maximum is held by two DIFFERENT source rows of a group: the kernel's rule (the lower position) and the
            # even split of torch's amax backward then agree (duplicates of one row tie, and there they do)
            assert FR.asap_tied_sources(d) == 0 and d["x_pool"].shape == d["x"].shape
            assert d["alpha_mask"] is None or d["alpha_mask"].shape == (d["edge_index"].size(1),)
        if family == "maxcut":
            assert d["kept"].numel() > 0 and 0 <= int(d["kept"].min()) and int(d["kept"].max()) < d["n"]
            assert d["s"].shape == (d["n"],) and bool((d["s"] > 0).all())


@pytest.mark.parametrize("family", sorted(FLOAT_REFS))
def test_the_reference_alone_is_well_conditioned(family):
    """e(r32) <= CAP / FACTOR for every float output of every seed (values); the float32 restatement as the product
    passes ``grad_path_errors``, whose bound may not exceed CAP (gradients)."""
    ref = FLOAT_REFS[family]
    for d in draws(family.split("_")[0]):
        with torch.no_grad():
            r64, r32 = ref(d, torch.float64)[0], ref(d, torch.float32)[0]
        worst = conditioning(r64, r32)
        assert worst <= CAP / FACTOR, (family, d["seed"], worst)
        # (the upstream gradients are seeded by the case's name: the public layer of the two edge families is checked
        # under the names the sweep uses, so this is the conditioning of exactly the gradients compared on the device)
        case = f"{family}-public-{d['seed']}" if family in ("asap", "maxcut") else f"{family}-{d['seed']}"
        fails = forward_errors(case, r32, r64, r32)
        fails += grad_path_errors(case, lambda: ref(d, torch.float32), lambda dt: ref(d, dt), LEAVES[family])
        assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", ["kmis", "edge_contract"])
def test_the_selector_references_pass_themselves(family):
    exact = FR.kmis_exact if family == "kmis" else FR.edge_contract_exact
    for d in draws(family)[::4]:
        want = exact(d)
        assert not forward_errors(f"{family}-{d['seed']}", exact(d), want, want, exact=set(want))
        n = d["n"]
        assert want["cluster"].numel() == n and (n == 0 or int(want["cluster"].max()) == int(want["k"]) - 1)


# ------------------------------------------------------------------------------------------------ stand-in faults
def _flagged(fails):
    return {m.split("output ")[1].split(":")[0] for m in fails if "output " in m}


def test_a_dropped_last_row_of_a_64_row_block_is_flagged():
    """A wrong Python stand-in for the Just Balance pass: row 63 of every 64-row block of a graph is never added."""
    part, hits = limits()["part_rows"], 0
    for d in draws("jb"):
        r64, r32 = FR.jb_reference(d, torch.float64)[0], FR.jb_reference(d, torch.float32)[0]
        s = d["s"].clone()
        for b in range(d["B"]):
            FR.jb_rows(d, s, b)[part - 1::part] = 0  # (a view: the rows of graph b)
        bad = FR.jb_reference(d, torch.float32, s=s)[0]
        fails = forward_errors(f"jb-{d['seed']}", bad, r64, r32)
        every_row = d["layout"] in ("mask_holes", "mask_empty_row")  # (all N rows of S count there)
        hit = {f"term[{b}]" for b in FR.jb_finite(d) if (d["N"] if every_row else d["sizes"][b]) >= part}
        assert _flagged(fails) == hit, (d["seed"], fails)
        hits += bool(hit)
    assert hits >= 1


def test_a_tie_resolved_to_the_higher_index_is_flagged():
    """A wrong stand-in for the k-MIS order: among equal scores the HIGHER node goes first."""
    hits = 0
    for d in draws("kmis"):
        want = FR.kmis_exact(d, perm=FR.tied_order(d["score"]))
        bad = FR.kmis_exact(d, perm=FR.tied_order(d["score"], higher=True))
        fails = forward_errors(f"kmis-{d['seed']}", bad, want, want, exact=set(want))
        if fails:
            assert _flagged(fails) & {"mis", "cluster"}, fails
            hits += 1
    assert hits >= 1


def test_a_quantile_held_by_the_higher_row_is_flagged():
    """A wrong stand-in for the quantile select: among the rows that hold a column's quantile value the HIGHEST is
    reported; the rule is "the lowest row holds it"."""
    hits = 0
    for d in draws("acc"):
        want = FR.acc_quantile_exact(d)
        bad = FR.acc_quantile_exact(d, higher=True)
        fails = forward_errors(f"acc-{d['seed']}", bad, want, want, exact=set(want))
        if fails:
            assert _flagged(fails) == {"qnode"}, fails
            hits += 1
    assert hits >= 1


def test_one_loss_term_scaled_by_a_thousandth_is_flagged():
    """A wrong stand-in: the float64 restatement with ONE graph's term times 1 + 1e-3, in the value and in the gradient."""
    hits = 0
    for d in draws("jb"):
        if not FR.jb_finite(d):
            continue
        r64, r32 = FR.jb_reference(d, torch.float64)[0], FR.jb_reference(d, torch.float32)[0]

        def faulty(dtype=torch.float64):
            outs, lv = FR.jb_reference(d, dtype)
            return {n: (v * (1 + 1e-3) if n == name else v) for n, v in outs.items()}, lv
        name = sorted(r64)[-1]
        case = f"jb-{d['seed']}"
        fails = forward_errors(case, faulty()[0], r64, r32)
        assert _flagged(fails) == {name}, (d["seed"], fails)
        gfails = grad_path_errors(case, faulty, lambda dt: FR.jb_reference(d, dt), ["s"])
        assert gfails and all(f"path {name}," in m for m in gfails), gfails
        hits += 1
    assert hits >= 1


# ------------------------------------------------------------------------------------------- ASAP and MaxCut stand-ins
def test_the_exact_references_of_the_edge_families_pass_themselves():
    """The index, the arg-max table and the labels are deterministic functions of the draw, and the two index forms of
    one direction describe the same groups in the same order."""
    for d in draws("asap")[::4] + draws("maxcut")[::4]:
        ei, n = d["edge_index"], d["n"]
        for by_dst in (True, False):
            want = FR.edge_group_exact(ei, n, by_dst)
            assert int(want["row_ptr"][-1]) == ei.size(1) and want["max_members"] == int(want["row_ptr"].diff().max())
            order = FR.regrouped_order(ei, by_dst)
            other = FR.edge_group_exact(ei[:, order], n, by_dst)
            assert torch.equal(other["row_ptr"], want["row_ptr"])
            pos = lambda g, m: torch.arange(m) if g["perm"] is None else g["perm"]  # noqa: E731
            assert torch.equal(order[pos(other, ei.size(1))], pos(want, ei.size(1)))  # the same edges in the same order
    for d in draws("asap")[::4]:
        want = FR.asap_argmax_exact(d)
        assert not forward_errors(f"asap-{d['seed']}", FR.asap_argmax_exact(d), want, want, exact=set(want))
        if d["edge_index"].size(1):
            src = d["edge_index"][0][want["argpos"].clamp(min=0)]
            picked = torch.where(want["argpos"] >= 0, d["x_pool"][src, torch.arange(d["F"]).expand_as(src)], 0.0)
            assert torch.equal(picked, want["max"])  # the maximum is the entry at the stored position
    for d in draws("maxcut")[::4]:
        label = FR.maxcut_labels_exact(d)
        assert torch.equal(label[d["kept"]], torch.arange(1, d["kept"].numel() + 1))


def test_an_argmax_tie_resolved_to_the_higher_position_is_flagged():
    """A wrong stand-in for ASAP's master query: among equal maxima the HIGHER edge position is stored.  Duplicate edges
    tie in every column, the tied rows of ``x_tied`` between different sources; the maximum itself is the same."""
    hits = 0
    for d in draws("asap"):
        for rows in [d["x_pool"]] + ([d["x_tied"]] if d["x_tied"] is not None else []):
            want, bad = FR.asap_argmax_exact(d, rows), FR.asap_argmax_exact(d, rows, higher=True)
            fails = forward_errors(f"asap-{d['seed']}", bad, want, want, exact=set(want))
            if fails:
                assert _flagged(fails) == {"argpos"}, fails
                hits += 1
    assert hits >= 1


def test_an_edge_softmax_that_loses_the_65th_edge_of_a_group_is_flagged():
    """A wrong stand-in for ASAP's edge softmax: lane 0's second trip through a group never reaches the sum.  Flagged as
    "alpha" on exactly the draws with a group of at least 65 edges."""
    hits = 0
    for d in draws("asap"):
        inp = FR.asap_operator_inputs(d)
        with torch.no_grad():
            r64, r32 = (FR.asap_operator_reference(d, dt, inp)[0] for dt in (torch.float64, torch.float32))
            bad = FR.asap_operator_reference(d, torch.float32, inp, drop_65th=True)[0]
        fails = forward_errors(f"asap-{d['seed']}", bad, r64, r32)
        assert _flagged(fails) == ({"alpha"} if d["in_degree_max"] >= 65 else set()), (d["seed"], fails)
        hits += bool(fails)
    assert hits >= 1


def test_a_diagonal_term_at_or_above_n_p_is_flagged():
    """A wrong stand-in for MaxCut's layer: every node gets (1 - delta) z_i, also those at or above n_P (which the
    reference's matrix has no row for).  Flagged as the layers' outputs on exactly the draws whose list does not reach N."""
    hits = 0
    for d in draws("maxcut"):
        inp = FR.maxcut_operator_inputs(d)
        with torch.no_grad():
            r64, r32 = (FR.maxcut_operator_reference(d, dt, inp)[0] for dt in (torch.float64, torch.float32))
            bad = FR.maxcut_operator_reference(d, torch.float32, inp, n_p=d["n"])[0]
        fails = forward_errors(f"maxcut-{d['seed']}", bad, r64, r32)
        layers = {f"{name}{l}" for l in range(len(d["widths"])) for name in ("h", "lin")} \
            | {f"z_next{l}" for l in range(len(d["widths"]) - 1)}
        if d["n_p"] < d["n"]:
            assert _flagged(fails) and _flagged(fails) <= layers and f"lin0" in _flagged(fails), (d["seed"], fails)
            hits += 1
        else:
            assert not fails, (d["seed"], fails)
    assert hits >= 1
