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
* GTVConv ("gtv"): every draw keeps the three margins of its separation rule (no draw is given up), and two wrong
  stand-ins for the backward operators -- a ``dh`` without the 65th in-edge's term, a ``g`` with the relu slope of the
  neighbouring row -- are flagged where the draw can show them.
* PAN ("pan"): every draw keeps a gap between the kept and the dropped scores of each graph and its pooled values clear
  of the Connect's eps filter; a MET fill that drops zero-valued entries and a ``part`` that stops at a row's 64th stored
  entry are flagged.
* EigenPooling ("eigenpool"): the groups whose modes keep the invariants alone are at most 5 % of all groups; a Reduce that
  drops a group's 129th row, one whose second wave starts a row late and modes with two columns swapped are flagged.
"""
import pytest
import torch

import fuzz_inputs as FI
import fuzz_refs as FR
import gtv_restatement as R_GTV
from fuzz_compare import CAP, FACTOR, conditioning, forward_errors, grad_path_errors

_LIMITS = {}


def limits():
    """The library's limits, read on first use: a tree without the built library fails its tests, not the collection."""
    if not _LIMITS:
        _LIMITS.update(FI.library_limits())
    return _LIMITS


def _dmon_raw(d):
    return d["s"].transpose(1, 2) @ d["adj"] @ d["s"]


_PAN_EXACT = {}


def _pan_exact(d):
    """The exact outputs of a PAN draw (the float64 selection among them), computed once per seed."""
    if d["seed"] not in _PAN_EXACT:
        _PAN_EXACT[d["seed"]] = FR.pan_exact(d)
    return _PAN_EXACT[d["seed"]]


FLOAT_REFS = {"jb": FR.jb_reference, "readout": FR.readout_reference, "sag": FR.sag_reference,
              "bnpool": FR.bnpool_reference, "bnpool_operators": FR.bnpool_operator_reference,
              "dmon": lambda d, dt: FR.dmon_reference(d, dt, _dmon_raw(d), grads=True),
              "acc": FR.acc_reference,
              "lapool": lambda d, dt: FR.lapool_reference(d, dt, FR.lapool_leaders(d, FR.lapool_variation(d, torch.float32))),
              "acc_flat": lambda d, dt: FR.acc_flat_reference(d, dt) if d["prefix"] else ({}, {}),
              "hosc": lambda d, dt: FR.hosc_reference(d, dt, _dmon_raw(d) if d["with_raw"] else None, grads=True),
              "asap": FR.asap_reference, "asap_operators": FR.asap_operator_reference,
              "maxcut": FR.maxcut_reference, "maxcut_operators": FR.maxcut_operator_reference,
              "gtv": FR.gtv_reference, "gtv_operators": FR.gtv_operator_reference,
              "gtv_dense": lambda d, dt: FR.gtv_dense_reference(d, dt) if d["dense"] else ({}, {}),
              "pan": lambda d, dt: FR.pan_reference(d, dt, _pan_exact(d)), "pan_operators": FR.pan_operator_reference,
              "eigenpool": FR.eigenpool_reference, "eigenpool_operators": FR.eigenpool_operator_reference}
# the names the sweep gives its cases on the device, where they differ from "<family>-<seed>": the upstream gradients are
# seeded by them
CASE_NAMES = {"asap": "asap-public-{}", "maxcut": "maxcut-public-{}", "gtv": "gtv-public-{}",
              "gtv_dense": "gtv-public-{}-dense", "gtv_operators": "gtv-op-{}", "pan": "pan-public-{}",
              "pan_operators": "pan-op-{}", "eigenpool": "eigenpool-public-{}", "eigenpool_operators": "eigenpool-op-{}"}
ASAP_PARAMS = ["lin.weight", "lin.bias", "att.weight", "att.bias", "select_scorer.lin1.weight", "select_scorer.lin1.bias",
               "select_scorer.lin2.weight", "select_scorer.lin3.weight", "select_scorer.lin3.bias"]
# (every name a drawn score net can have: 1 ... 4 layers, a tail of up to two Linear; a leaf a draw lacks is skipped)
MAXCUT_PARAMS = [FR.RM.PRE + n + e for n in ["initial_layer", "final_layer", "mlp.0", "mlp.1"] for e in (".weight", ".bias")] \
    + [f"{FR.RM.PRE}mp_convs.{l}{e}" for l in range(4) for e in (".lin.weight", ".bias")]
LEAVES = {"jb": ["s"], "readout": ["x", "weight"], "sag": ["x", "w_rel", "w_root", "b"], "bnpool": ["s", "k_mat"],
          "bnpool_operators": ["t", "s"], "dmon": ["s", "raw"], "hosc": ["s", "raw"], "acc": ["s"],
          "acc_flat": ["s"], "lapool": ["x"], "asap": ["x", "x_pool"] + ASAP_PARAMS,
          "asap_operators": ["x", "x_pool", "sq_in", "sp_in", "val", "p"], "maxcut": ["x", "s"] + MAXCUT_PARAMS,
          "maxcut_operators": ["z0", "z1", "z2", "z3", "h_tail", "s"],
          "gtv": ["x", "weight", "bias", "edge_weight"], "gtv_operators": ["h", "edge_weight"],
          "gtv_dense": ["x", "weight", "bias"], "pan": ["x", "weight", "lin.weight", "lin.bias", "p", "beta"],
          "pan_operators": ["c"], "eigenpool": ["x"], "eigenpool_operators": []}


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


def _degrees(d):
    """(out-degree, in-degree) [n] over the edges the kernels do not skip."""
    ei = d["edge_index"][:, ~FR.gtv_skipped(d)]
    return torch.bincount(ei[0], minlength=d["n"]), torch.bincount(ei[1], minlength=d["n"])


def _gtv_coverage(ds):
    from tgp import kernels as K
    lim = limits()
    reg = lim["gtv_register_channels"]
    assert reg == K.GTV_REGISTER_CHANNELS and {reg, reg + 1, reg + 4} <= set(FI.GTV_WIDTHS)
    assert set(FI.GTV_ACT_NAMES) == set(K.GTV_ACT_CODES)
    assert sorted(d["C"] for d in ds) == sorted(FI.GTV_WIDTHS) and len(FI.GTV_WIDTHS) == len(FI.SEEDS)
    # both load forms on each side of every switch of the register kernels, and the chunked kernels past them
    for lo, hi in ((32, 33), (64, 65), (128, 129), (256, 257), (reg, reg + 1)):
        assert FI.gtv_layout_class(lo, lim) != FI.gtv_layout_class(hi, lim)
    forms = {(FI.gtv_layout_class(d["C"], lim), d["form"]) for d in ds}
    assert forms >= {(k, f) for k in ((8, 4), (16, 4), (32, 4), (64, 4), (64, 8)) for f in ("vec16", "scalar")}
    assert any(k == "chunked" for k, _ in forms)
    for d in ds:
        assert d["form"] == ("vec16" if d["C"] % 4 == 0 and d["layout"] == "plain" else "scalar")
    assert any(d["layout"] == "offset" and d["C"] % 4 == 0 for d in ds)  # a width that loses the 16-byte loads to its base
    assert {d["layout"] for d in ds} == set(FI.LAYOUTS["gtv"])
    # graph sizes around the nodes of a block at the drawn width; 1 and 2; batches of 1 .. 5
    assert {d["block_nodes"] for d in ds} == {4, 8, 16, 32}
    for d in ds:
        cls = FI.gtv_layout_class(d["C"], lim)
        assert d["block_nodes"] == (4 if cls == "chunked" else 256 // cls[0])
        assert len(d["sizes"]) == d["B"] and d["n"] == sum(d["sizes"]) and min(d["sizes"]) >= 1
        assert d["C"] <= 256 or d["n"] <= 40
    for p in (4, 8, 16, 32):
        assert {p - 1, p, p + 1} <= {v for d in ds if d["block_nodes"] == p for v in d["sizes"]}
    assert {1, 2} <= {v for d in ds for v in d["sizes"]} and {d["B"] for d in ds} == set(FI.GTV_BATCHES)
    # the hubs: exact degrees over the edges the kernels walk, the in-hub with one out-edge
    assert {d["out_hub"] for d in ds} == set(FI.GTV_OUT_HUBS) and {d["in_hub"] for d in ds} == set(FI.GTV_IN_HUBS)
    for d in ds:
        out, inn = _degrees(d)
        assert int(out[d["out_hub_node"]]) == d["out_hub"], d["seed"]
        assert int(inn[d["in_hub_node"]]) == d["in_hub"] and int(out[d["in_hub_node"]]) == 1, d["seed"]
    assert any(int((_degrees(d)[1] > _degrees(d)[0]).sum()) > 0 for d in ds)  # more in-edges than out-edges
    # the list: three orders, so that either index has both forms; duplicates, loops, weights with exact zeros
    assert {d["order"] for d in ds} == set(FI.EDGE_ORDERS)
    forms = {(by_dst, FR.edge_group_exact(d["edge_index"], d["n"], by_dst)["perm"] is None) for d in ds for by_dst in (True, False)}
    assert forms == {(True, True), (True, False), (False, True), (False, False)}
    long_in = {FR.edge_group_exact(d["edge_index"], d["n"], True)["perm"] is None for d in ds if d["in_hub"] >= 65}
    assert long_in == {True, False}  # the long in-edge loop with and without a permutation
    assert {d["dups_loops"] for d in ds} == {True, False} and {d["weighted"] for d in ds} == {True, False}
    assert any(bool(FR.gtv_skipped(d).any()) for d in ds)
    assert any(torch.unique(d["edge_index"], dim=1).size(1) < d["edge_index"].size(1) for d in ds)
    assert any(d["edge_weight"] is not None and bool((d["edge_weight"] == 0).any()) for d in ds)
    assert {d["edge_weight"] is None for d in ds} == {True, False}
    assert {d["mask"] is not None for d in ds} == {True, False}
    assert any(d["mask"] is not None and 0 < int(d["mask"].sum()) < d["n"] for d in ds)
    assert {d["mask"] is not None for d in ds if d["act"] == "relu"} == {True, False}
    assert {d["act"] for d in ds} == set(FI.GTV_ACT_NAMES) and {d["delta"] for d in ds} == set(FI.GTV_DELTAS)
    assert {d["eps"] for d in ds} == set(FI.GTV_EPS) and {d["bias"] is not None for d in ds} == {True, False}
    assert sum(d["dense"] for d in ds) == 2
    for d in ds:  # eps = 0.5 clamps a share of the edges (an equal pair among them), eps = 1e-3 none of the twins
        dist = R_GTV.distances(d["h"].double(), d["edge_index"])[1]
        clamped = int((dist < d["eps"]).sum())
        assert (0 < clamped < dist.numel() or d["C"] == 1) if d["eps"] == 0.5 else clamped == 0, (d["seed"], clamped)
        assert d["eps"] != 0.5 or float(dist.min()) == 0.0
        assert float(dist.min()) < 0.25  # a twin pair: d_e well under the width's typical distance


def _pan_coverage(ds):
    lim = limits()["pan_max_graph_nodes"]
    assert {v for d in ds for v in d["sizes"]} >= set(FI.PAN_SIZES) | {lim - 1, lim, lim + 1}
    assert {d["B"] for d in ds} == set(FI.PAN_BATCHES) and all(len(d["all_sizes"]) == d["B"] + 1 for d in ds)
    assert {d["filter_size"] for d in ds} == set(FI.PAN_FILTERS) and {d["weights"] for d in ds} == set(FI.PAN_WEIGHTS)
    assert {d["directed"] for d in ds} == {True, False} and {d["order"] for d in ds} == {"by_source", "shuffled"}
    assert {d["hub"] for d in ds} == set(FI.PAN_HUB_ENTRIES)
    assert {d["route"] for d in ds} == {"native", "composed"}
    for d in ds:
        big = max(d["sizes"]) >= lim - 1
        assert d["route"] == ("composed" if max(d["all_sizes"]) > lim else "native")
        assert not big or 1 <= d["filter_size"] <= 2
        assert d["weight"].shape == (d["filter_size"] + 1,)
        w = d["weight"].abs()
        assert bool(((w >= 0.4) & (w <= 0.9) | (w == 0)).all())
        assert int((d["weight"] == 0).sum()) == (d["weights"] == "zero") and int((d["weight"] < 0).sum()) == (d["weights"] == "negative")
        # the planted row stores exactly ``hub`` entries, every other node of the hub within filter_size hops of it
        ex = FR.pan_exact(d)
        assert int((ex["index"][0] == d["hub_row"]).sum()) == d["hub"], d["seed"]
        assert pan_gap(d, ex) >= FI.PAN_GAP, d["seed"]
        # the Connect's filter |value| > eps decides on exact zeros alone: every other pooled value is far above eps
        rest = ex["pooled_all"][ex["pooled_all"] != 0].abs()
        assert bool((ex["pooled_all"][~ex["pooled_stored"]] == 0).all()) and (rest.numel() == 0 or float(rest.min()) > 1e-6)
        # the scorer: one node's column group holds exactly the drawn number of entries
        assert int((d["score_index"][1] == d["score_node"]).sum()) == d["score_group"]
        assert d["score_x"].shape == (d["n"], d["score_F"])
    assert any(bool((d["edge_index"][0] == d["edge_index"][1]).any()) for d in ds)  # loops
    assert any(torch.unique(d["edge_index"], dim=1).size(1) < d["edge_index"].size(1) for d in ds)  # multi-edges
    assert {d["score_F"] for d in ds} == set(FI.PAN_SCORE_FEATURES) and {d["score_group"] for d in ds} == set(FI.PAN_SCORE_GROUPS)
    assert {d["layout"] for d in ds} == set(FI.LAYOUTS["pan"]) and {d["use_tanh"] for d in ds} == {True, False}
    assert {FI.PAN_SCORE_LANES - 1, FI.PAN_SCORE_LANES, FI.PAN_SCORE_LANES + 1} <= set(FI.PAN_SCORE_FEATURES) & set(FI.PAN_SCORE_GROUPS)
    # rows on either side of 64 stored entries reach the backward with a series of several terms
    native = [d for d in ds if d["route"] == "native"]
    assert {d["hub"] for d in native if d["filter_size"] >= 1} >= {63, 64, 65, 129}


def _eigenpool_coverage(ds):
    lim = limits()["eigenpool_max_group_nodes"]
    assert FR.EIG_GAP == FI.EIG_GAP
    assert {d["H"] for d in ds} == set(FI.EIG_MODES) and {d["normalized"] for d in ds} == {True, False}
    assert {c for d in ds for c in d["classes"]} == set(FI.EIG_SIZE_CLASSES)
    sizes = {m for d in ds for c in d["clusters"] for m in c}
    assert {1, 2, 3, lim - 1, lim, lim + 1} <= sizes
    assert any(20 <= m <= 40 and m % 2 == 0 for m in sizes) and any(20 <= m <= 40 and m % 2 == 1 for m in sizes)
    for d in ds:  # around the drawn H; several groups per graph, interleaved in node order, an empty one in the middle
        for name, m in zip(d["classes"], [d["clusters"][0][0], d["clusters"][0][2], d["clusters"][1][0], d["clusters"][1][1]]):
            assert {"H-1": max(d["H"] - 1, 1), "H": d["H"], "H+1": d["H"] + 1}.get(name, m) == m
        assert d["clusters"][0][1] == 0 and len(d["clusters"]) == 2 and all(len(c) == d["width"] for c in d["clusters"])
        counts = torch.bincount(d["gid"], minlength=2 * d["width"]).view(2, -1).tolist()
        assert counts == d["clusters"]
        lab = d["labels"][: d["sizes"][0]]
        assert d["sizes"][0] < 3 or bool((lab[1:] < lab[:-1]).any())  # not sorted by cluster
        a = torch.zeros(d["n"], d["n"]).index_put((d["edge_index"][0], d["edge_index"][1]), d["edge_weight"])
        assert torch.equal(a, a.t()) and float(d["edge_weight"].min()) > 0 and d["edge_weight"].unique().numel() > 1
        assert bool((d["gid"][d["edge_index"][0]] != d["gid"][d["edge_index"][1]]).any())  # edges between clusters
    # Reduce and Lift: the longest group on either side of both thresholds, the others short or empty, every F and H
    assert {d["longest"] for d in ds} == set(FI.EIG_LONGEST) and {d["F"] for d in ds} == set(FI.EIG_FEATURES)
    assert {FI.EIG_REDUCE_ONE_WAVE + k for k in (-1, 0, 1)} | {FI.EIG_REDUCE_FOUR_WAVES + k for k in (-1, 0, 1)} == set(FI.EIG_LONGEST)
    assert {d["reduce_H"] for d in ds} == set(FI.EIG_REDUCE_MODES)
    assert {FI.EIG_MODE_CHUNK - 1, FI.EIG_MODE_CHUNK, FI.EIG_MODE_CHUNK + 1, 2 * FI.EIG_MODE_CHUNK + 1} <= set(FI.EIG_REDUCE_MODES)
    assert {d["layout"] for d in ds} == set(FI.LAYOUTS["eigenpool"]) and sum(d["hints"] for d in ds) == 4
    for d in ds:
        rows = torch.bincount(d["reduce_gid"], minlength=d["reduce_groups"]).tolist()
        assert rows == d["rows"] and max(rows) == d["longest"] and set(rows) - {d["longest"]} <= set(FI.EIG_OTHER_ROWS)
        assert set(FI.EIG_OTHER_ROWS) <= set(rows)
        assert not torch.equal(torch.sort(d["reduce_gid"]).values, d["reduce_gid"])  # interleaved in node order
    waves = lambda n: 1 if n <= FI.EIG_REDUCE_ONE_WAVE else (4 if n <= FI.EIG_REDUCE_FOUR_WAVES else 16)  # noqa: E731
    shared = [d["longest"] for d in ds if waves(d["longest"]) > 1]
    assert {waves(n) for n in shared} == {4, 16}
    assert any(-(-n // waves(n)) % FI.EIG_ROW_UNROLL for n in shared)  # a per-wave range that is no multiple of the unroll
    assert any(n % waves(n) for n in shared)                           # a clipped last range


def test_eigen_groups_left_to_the_invariants_are_at_most_a_twentieth():
    """From the float64 reference alone: the groups with a spectral gap or a sign-fixing entry under EIG_GAP, or a float32
    restatement beyond CAP / FACTOR, are at most 5 % of the groups of the 16 seeds."""
    good = rest = 0
    for d in draws("eigenpool"):
        g, r = FR.eigenpool_compared_groups(d)
        good, rest = good + len(g), rest + len(r)
    assert rest <= 0.05 * (good + rest), (rest, good)


def pan_gap(d, ex):
    """The distance between the kept and the dropped scores of the float64 reference (``ex``: its exact outputs): the
    scorer's definition on the reference's own conv_out and M, whose entries at the kept nodes are the reference's."""
    import pan_restatement as RP
    with torch.no_grad():
        outs, _ = FR.pan_reference(d, torch.float64, ex)
    full = torch.tanh(RP.raw_score(outs["conv_out"], ex["index"], outs["met_values"], d["p"].double(), d["beta"].double()))
    assert torch.equal(full[ex["kept"]], outs["weight"])
    return FI.pan_cut_gap(full, d["batch"], d["all_sizes"])


@pytest.mark.parametrize("family", FI.FAMILIES)
def test_every_boundary_value_layout_and_route_is_drawn(family):
    ds = draws(family)
    if family == "gtv":
        return _gtv_coverage(ds)
    if family == "pan":
        return _pan_coverage(ds)
    if family == "eigenpool":
        return _eigenpool_coverage(ds)
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
        if family == "gtv":
            E = d["edge_index"].size(1)
            assert d["h"].shape == (d["n"], d["C"]) and d["x"].shape == (d["n"], FI.GTV_F_IN) and E > 0
            assert d["weight"].shape == (FI.GTV_F_IN, d["C"]) and d["batch"].numel() == d["n"] == int(d["ptr"][-1])
            assert d["edge_weight"] is None or d["edge_weight"].shape == (E,)
            assert d["mask"] is None or (d["mask"].shape == (d["n"],) and d["mask"].dtype == torch.bool)


@pytest.mark.parametrize("seed", FI.SEEDS)
def test_gtv_draws_keep_the_kinks_away(seed):
    """The separation rule holds on every draw, in float64 and for both layers: no channel difference of an edge in
    (0, GTV_MARGIN), no distance within GTV_MARGIN eps of eps, for relu no pre-activation of a kept row within GTV_MARGIN
    of 0 -- also in dense mode, whose padded rows are masked.  ``draw`` raises rather than give a seed up."""
    d = FI.draw("gtv", seed, limits())
    assert 0 <= d["sub_seed"] < FI.GTV_SUB_SEEDS
    layers = [(d["h"].double(), d["mask"]), (d["x"].double() @ d["weight"].double(), None)]
    for h, mask in layers:
        gap, near, pre = FI.gtv_margins(h, d["edge_index"], d["edge_weight"], d["bias"], mask, d["delta"], d["eps"], d["act"])
        assert gap >= FI.GTV_MARGIN and near >= FI.GTV_MARGIN and pre >= FI.GTV_MARGIN, (seed, gap, near, pre)
    if d["dense"]:
        x, adj, mask = FR.gtv_dense_batch(d)
        ei, w = R_GTV.dense_edges(adj)
        h = (x.double() @ d["weight"].double()).reshape(-1, d["C"])
        gap, near, pre = FI.gtv_margins(h, ei, w, d["bias"], mask.reshape(-1), d["delta"], d["eps"], d["act"])
        assert gap >= FI.GTV_MARGIN and near >= FI.GTV_MARGIN and pre >= FI.GTV_MARGIN, (seed, gap, near, pre)


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
        case = CASE_NAMES.get(family, family + "-{}").format(d["seed"])
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


# ---------------------------------------------------------------------------------------------------- GTVConv stand-ins
def _gtv_by_graph(d, outs):
    """``outs`` plus the rows of "g" and "dh" graph by graph, as the sweep compares them."""
    res = dict(outs)
    for name in ("g", "dh"):
        for b in range(d["B"]):
            res[f"{name}[{b}]"] = outs[name][int(d["ptr"][b]):int(d["ptr"][b + 1])]
    return res


def _gtv_hand_made(d, **fault):
    """(failures of the hand-made backward against autograd's, the float64 hand-made outputs)."""
    with torch.no_grad():
        r64, r32 = (_gtv_by_graph(d, {k: v for k, v in FR.gtv_operator_reference(d, dt)[0].items() if k in ("g", "dh")})
                    for dt in (torch.float64, torch.float32))
        bad = _gtv_by_graph(d, FR.gtv_backward_by_hand(d, torch.float32, **fault))
    return forward_errors(f"gtv-op-{d['seed']}", bad, r64, r32)


def test_a_dh_without_the_65th_in_edge_is_flagged():
    """The backward operators' formulas written out by hand pass against autograd on every draw; the same with the 65th
    in-edge of every node left out of dh is flagged as "dh" (and as the hub's graph) on exactly the draws where a node
    has 65 in-edges whose 65th carries a term, and nowhere else."""
    hits = 0
    for d in draws("gtv"):
        assert not _gtv_hand_made(d), d["seed"]
        rank, keep = FR.gtv_in_edge_rank(d), ~FR.gtv_skipped(d)
        lost = d["edge_index"][:, keep & (rank == 64)]
        good = FR.gtv_backward_by_hand(d, torch.float64)["dh"]
        gone = FR.gtv_backward_by_hand(d, torch.float64, drop_in_edge=65)["dh"]
        fails = _gtv_hand_made(d, drop_in_edge=65)
        if lost.size(1) and float((good - gone).abs().max()) > 1e-3 * float(good.abs().max()):
            graphs = {f"dh[{int(d['batch'][j])}]" for j in lost[1].tolist()}
            assert "dh" in _flagged(fails) and graphs <= _flagged(fails) <= {"dh"} | graphs, (d["seed"], fails)
            hits += 1
        elif not lost.size(1):
            assert not fails and torch.equal(good, gone), (d["seed"], fails)
    assert hits >= 2  # (in-degrees 65 and 257 are both drawn)


def test_a_relu_slope_from_the_neighbouring_row_is_flagged():
    """A wrong stand-in for the terms kernel: g_i = upstream_i relu'(out_{i+1}).  Flagged as "g" on every relu draw (dh,
    which is built from g, goes with it); identity has one slope everywhere and shows nothing."""
    hits = 0
    for d in draws("gtv"):
        fails = _gtv_hand_made(d, slope_from_next_row=True)
        if d["act"] == "relu":
            assert "g" in _flagged(fails), (d["seed"], fails)
            hits += 1
        elif d["act"] == "identity":
            assert not fails, (d["seed"], fails)
    assert hits >= 2


# -------------------------------------------------------------------------------------------------------- PAN stand-ins
def _pan_operator_pair(d):
    with torch.no_grad():
        return (FR.pan_operator_reference(d, dt)[0] for dt in (torch.float64, torch.float32))


def test_a_met_whose_zero_weight_removes_entries_is_flagged():
    """A wrong stand-in for the MET fill: entries whose value is 0 are not stored.  The pattern is structural, so a zero
    weight (every coefficient from it on is 0) must keep the entries only longer walks reach: flagged as "index" on the
    draws with a zero weight that have such entries, and on no other."""
    hits = 0
    for d in draws("pan"):
        ex = FR.pan_exact(d)
        r64, r32 = _pan_operator_pair(d)
        stored = r32["values"] != 0
        bad = {"index": ex["index"][:, stored], "values": r32["values"][stored]}
        want = {"index": ex["index"], "values": r64["values"]}
        fails = forward_errors(f"pan-op-{d['seed']}", bad, want, {"values": r32["values"]}, exact={"index"})
        if d["weights"] == "zero" and not bool(stored.all()):
            assert "index" in _flagged(fails), (d["seed"], fails)
            hits += 1
        else:
            assert bool(stored.all()) and not fails, (d["seed"], fails)
    assert hits >= 1


def test_a_part_that_stops_at_the_64th_stored_entry_is_flagged():
    """A wrong stand-in for ``pan_met_bwd``: a row's walk ends after its first 64 stored entries.  Flagged as "part" (and
    "dc", its column sums) on exactly the draws with a row of more than 64 entries and a series beyond its first term."""
    hits = 0
    for d in draws("pan"):
        r64, r32 = _pan_operator_pair(d)
        with torch.no_grad():
            bad = dict(r32, part=FR.pan_operator_reference(d, torch.float32, row_limit=64)[0]["part"])
        bad["dc"] = bad["part"].sum(0)
        fails = forward_errors(f"pan-op-{d['seed']}", bad, r64, r32)
        longest = int(torch.bincount(FR.pan_exact(d)["index"][0]).max())
        if longest > 64:
            assert "part" in _flagged(fails) and _flagged(fails) <= {"part", "dc"}, (d["seed"], fails)
            hits += 1
        else:
            assert not fails, (d["seed"], fails)
    assert hits >= 2


# ------------------------------------------------------------------------------------------------ EigenPooling stand-ins
def _eigenpool_faulty(d, **fault):
    with torch.no_grad():
        r64, r32 = (FR.eigenpool_operator_reference(d, dt)[0] for dt in (torch.float64, torch.float32))
        bad = FR.eigenpool_operator_reference(d, torch.float32, **fault)[0]
    return _flagged(forward_errors(f"eigenpool-op-{d['seed']}", bad, r64, r32))


def test_a_reduce_that_drops_row_129_of_a_group_is_flagged():
    """A wrong stand-in for the Reduce: the 129th row of a group never reaches the sum.  Flagged as "pool" on exactly the
    draws whose longest group has at least 129 rows -- the 129-row groups among them."""
    hits = 0
    for d in draws("eigenpool"):
        assert _eigenpool_faulty(d, drop_row=129) == ({"pool"} if d["longest"] >= 129 else set()), d["seed"]
        hits += d["longest"] == 129
    assert hits >= 1


def test_a_reduce_whose_second_wave_starts_one_row_late_is_flagged():
    """A wrong stand-in for the 4-wave Reduce: wave 1 starts at row per + 1 instead of per = ceil(len / 4).  Flagged as
    "pool" on every draw (the short groups lose a row as well: every group with more than one row has a row ``per``)."""
    for d in draws("eigenpool"):
        assert _eigenpool_faulty(d, late_wave=4) == {"pool"}, d["seed"]


def test_modes_with_two_columns_swapped_are_flagged():
    """A wrong stand-in for the modes kernel: the first two modes of every group change places.  Flagged as the modes of
    every compared group of more than one node where H >= 2; H = 1 has nothing to swap."""
    hits = 0
    for d in draws("eigenpool"):
        want = {f"modes[{g}]" for g in FR.eigenpool_compared_groups(d)[0] if int((d["gid"] == g).sum()) > 1} \
            if d["H"] >= 2 else set()
        assert _eigenpool_faulty(d, swap_modes=True) == want, d["seed"]
        hits += bool(want)
    assert hits >= 1
