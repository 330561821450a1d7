"""Seeded differential sweep of the newer kernel families against the float64 restatements.

Every test draws its inputs from tests/fuzz_inputs.py (16 seeds per family and layer: the smallest shapes at which a
kernel changes behaviour, every layout its wrapper accepts), runs the ``tgp.kernels`` wrappers (operator layer: the
forward and the native backward operator on the same upstream gradient) or the public functions and classes (public
layer: values per graph, gradients one output at a time) and compares with tests/fuzz_refs.py by the rule of
tests/fuzz_compare.py.  Integer outputs are compared with ``torch.equal``.  Each test asserts the route its draw was
made to reach where the wrapper reports one.  On one seed in four the same call runs twice (equal bits, forward and
backward) and the padded and the un-padded layout of the same batch are both held to the bound.

Every comparison prints a ``FUZZ`` line with e_kernel / e_r32; the worst ratios of the last measured run are in
profiles/fuzz_newer_families.txt.

Families: Just Balance, DMoN's, HOSC's and AsymCheegerCut's losses, LaPool's selector, BN-Pool's reconstruction loss, the
segment readout,
the SAG scorer, the k-MIS selector, the edge-contraction selector, ASAP's fitness (csrc/asap.hip) and MaxCut's score
net, cut loss and assignment rounds (csrc/maxcut.hip), and GTVConv's propagation (csrc/gtvconv.hip: the forward, then the
terms kernel and the node kernel of its backward called on their own, each on the one before's own results; widths on
both sides of every lane-group, register-count and chunking switch in both load forms, graph sizes around the nodes of a
block, one long out-edge and one long in-edge loop, inputs kept clear of the propagation's kinks by the draw), and PAN
(csrc/pan.hip: the MET matrix on graphs of 1 .. 129 nodes and at the node limit, one past it on the composed form; its
backward ``pan_met_bwd`` on its own, with a planted row of 1, 63, 64, 65 or 129 stored entries; the score kernel around
its 16 lanes in F and in a node's column group; ``PANConv`` -> ``PANPooling`` with the top-k cut kept clear of rounding),
and EigenPooling (csrc/eigenpool.hip: the modes kernel on groups of 1 node up to its limit and one past it, entries
compared where the float64 spectrum separates them and the invariants everywhere; Reduce and Lift with the longest group
on either side of the one-wave and the four-wave threshold among short and empty groups, every ``max_len`` class).
ASAP, MaxCut and GTVConv also compare the shared edge-group index (``kernels.sag_edge_group``, both directions, both
forms) exactly with a stable host argsort of the same list.
"""
import zlib

import pytest
import torch

import fuzz_inputs as FI
import fuzz_refs as FR
from fuzz_compare import factor_of, forward_errors, grad_path_errors, print_grad_report, print_report
from test_gpu_grad_paths import _graph_names

pytestmark = pytest.mark.gpu

SEEDS = list(FI.SEEDS)
F64, F32 = torch.float64, torch.float32


def dev():
    return torch.device("cuda:0")


def mv(t):
    return None if t is None else t.to(dev())


def limits():
    return FI.library_limits()


def offset_by_one_element(t):
    """The same values in a contiguous view that starts 4 bytes into its buffer (rows not 16-byte aligned)."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    out = buf[1:].view(t.shape)
    assert out.is_contiguous() and (t.numel() == 0 or out.data_ptr() % 16 == 4)
    return out


def upstream(case, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(zlib.crc32(case.encode())))


def finish(case, fails, report, kind="forward"):
    print_report(report, kind)
    assert not fails, "\n".join(fails)


def check_grads(case, kernel, oracle, leaves):
    report = []
    fails = grad_path_errors(case, kernel, oracle, leaves, report=report)
    print_grad_report(case, report)
    assert not fails, "\n".join(fails)
    return report


# ===================================================================================================== Just Balance
def _jb_inputs(d, layout=None):
    """(S on the device, the wrapper's keyword arguments, the batch vector of an un-padded S) for the drawn layout."""
    lay = d["layout"] if layout is None else layout
    if lay in ("ptr", "ptr_offset"):
        s = mv(d["s_flat"])
        if lay == "ptr_offset":
            s = offset_by_one_element(s)
        return s, dict(ptr=mv(d["ptr"]), max_nodes=max(d["sizes"])), mv(d["batch"])
    if lay == "sizes":
        return mv(d["s_padded"]), dict(graph_sizes=mv(torch.tensor(d["sizes"]))), None
    if lay == "mask_prefix":
        return mv(d["s_padded"]), dict(mask=mv(d["mask"])), None
    return mv(d["s"]), dict(mask=mv(d["mask"])), None


def _jb_view(d, layout):
    """The draw as the other layout of the same batch sees it (padded rows of S are zero there)."""
    v = dict(d)
    v["padded"] = layout in ("sizes", "mask_prefix")
    v["s"] = d["s_padded"] if v["padded"] else d["s_flat"]
    return v


def _jb_operator(d, case, layout, report, twice):
    from tgp import kernels as K
    v = _jb_view(d, layout) if "s_flat" in d else d
    s, kw, batch = _jb_inputs(d, layout)
    out, coef = K.jb_terms(s, **kw)
    assert out.dtype == F32 and tuple(out.shape) == (d["B"],) and tuple(coef.shape) == (d["B"], d["K"])
    fin = FR.jb_finite(v)
    for b in range(d["B"]):
        if b not in fin:
            assert float(out[b]) == float("-inf"), (case, b, float(out[b]))  # no real node: as the composed form
    r64, r32 = FR.jb_reference(v, F64)[0], FR.jb_reference(v, F32)[0]
    fails = forward_errors(case, FR.jb_split(v, out), r64, r32, factor=factor_of("jb"), report=report)
    # the native backward operator on the same upstream gradient, one graph at a time
    g = upstream(case, d["B"])
    g[[b for b in range(d["B"]) if b not in fin]] = 0
    ds = K.jb_ds(s, coef, mv(g), batch)
    assert ds.shape == s.shape

    def ref_grads(dtype):
        outs, lv = FR.jb_reference(v, dtype)
        if not outs:
            return {}
        total = sum(g[b].to(dtype) * outs[f"term[{b}]"] for b in fin)
        (gs,) = torch.autograd.grad(total, lv["s"])
        return {f"dS[{b}]": FR.jb_rows(v, gs, b) for b in fin}
    g64, g32 = ref_grads(F64), ref_grads(F32)
    got = {f"dS[{b}]": FR.jb_rows(v, ds.cpu(), b) for b in fin}
    fails += forward_errors(case, got, g64, g32, factor=factor_of("jb"), report=report)
    for b in fin:
        rows = got[f"dS[{b}]"]
        if d["zero_col"]:
            assert bool((rows[:, d["K"] // 2] == 0).all()), (case, b)  # c_k = 0: the coefficient stays finite
        if v["padded"] and layout in ("sizes", "mask_prefix"):
            assert bool((rows[d["sizes"][b]:] == 0).all()), (case, b)  # padded rows: exact zeros
    if twice:
        out2, coef2 = K.jb_terms(s, **kw)
        assert torch.equal(out, out2) and torch.equal(coef, coef2)
        # (equal_nan: the rows of a graph without a real node are 0 * inf)
        torch.testing.assert_close(K.jb_ds(s, coef2, mv(g), batch), ds, rtol=0, atol=0, equal_nan=True)
    return fails


@pytest.mark.parametrize("seed", SEEDS)
def test_jb_operators(seed):
    d = FI.draw("jb", seed, limits())
    case, report = f"jb-op-{seed}", []
    fails = _jb_operator(d, case, d["layout"], report, seed % 4 == 0)
    if seed % 4 == 0 and "s_flat" in d:  # the padded and the un-padded layout of the same batch, both within the bound
        other = "ptr" if d["padded"] else "sizes"
        fails += _jb_operator(d, f"{case}-as-{other}", other, report, False)
    finish(case, fails, report)


@pytest.mark.parametrize("seed", SEEDS)
def test_jb_public(seed):
    from tgp.utils.losses import jb_loss_terms, just_balance_loss, unbatched_just_balance_loss
    d = FI.draw("jb", seed, limits())
    case = f"jb-public-{seed}"
    fin = FR.jb_finite(d)
    keep = mv(FR.jb_row_mask(d))
    seen = {}

    def kernel():
        s, kw, batch = _jb_inputs(d)
        leaf = s.detach().clone().requires_grad_(True)
        s_in = torch.where(keep, leaf, leaf.detach())  # rows of a graph without a real node carry 0 * inf in every form
        if d["layout"] == "ptr_offset":
            s_in = offset_by_one_element(s_in)
        if d["padded"]:
            terms = jb_loss_terms(s_in, kw.get("mask"), kw.get("graph_sizes"))
        else:
            terms = jb_loss_terms(s_in, batch=batch)
        seen["terms"], seen["s"] = terms, s_in
        return FR.jb_split(d, terms), {"s": leaf}

    outs, _ = kernel()
    assert "_JBTermsFnBackward" in _graph_names(seen["terms"].grad_fn)
    report = []
    r64, r32 = FR.jb_reference(d, F64)[0], FR.jb_reference(d, F32)[0]
    fails = forward_errors(case, outs, r64, r32, factor=factor_of("jb"), report=report)
    # the reduced forms the public names hand out: the same terms, reduced in float32
    with torch.no_grad():
        if d["padded"] and d["layout"] != "sizes":
            total = just_balance_loss(seen["s"], mv(d["mask"]), batch_reduction="sum")
        elif not d["padded"]:
            total = unbatched_just_balance_loss(seen["s"], mv(d["batch"]), batch_reduction="sum")
        else:
            total = None
    if total is not None and len(fin) == seen["terms"].numel():
        want = {"sum": sum(r64.values())}
        fails += forward_errors(case, {"sum": total}, want, {"sum": sum(r32.values())}, factor=factor_of("jb"),
                                report=report)
    finish(case, fails, report)
    if fin:
        check_grads(case, kernel, lambda dt: FR.jb_reference(d, dt), ["s"])
    if seed % 4 == 0 and fin:  # the same public call twice: equal bits, forward and backward
        runs = []
        for _ in range(2):
            o, lv = kernel()
            total = sum(o.values())
            runs.append((seen["terms"].detach().clone(), torch.autograd.grad(total, lv["s"])[0]))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), case


# ============================================================================================================= DMoN
def _per_graph(name, t, graphs=None):
    return {f"{name}[{b}]": t[b] for b in (range(t.size(0)) if graphs is None else graphs)}


@pytest.mark.parametrize("seed", SEEDS)
def test_dmon_operators(seed):
    """``dmon_dense_terms`` (degrees and the per-block partial sums), ``dmon_node_terms`` and ``dmon_edge_degrees`` on
    the same batch un-padded, and the backward's elementwise ``dmon_ds``, each against its plain statement."""
    from tgp import kernels as K
    lim = limits()
    d = FI.draw("dmon", seed, lim)
    case, report, part_rows = f"dmon-op-{seed}", [], lim["part_rows"]
    s, adj, mask, sizes = mv(d["s"]), mv(d["adj"]), mv(d["mask"]), mv(d["graph_sizes"])
    deg, part = K.dmon_dense_terms(adj, s, mask, sizes)
    B, N, Kc = d["s"].shape
    assert tuple(part.shape) == (B, max(1, -(-N // part_rows)), 2 * Kc + 2)  # one block / the partial pass
    (d64, p64), (d32, p32) = FR.dmon_partial_sums(d, F64, part_rows), FR.dmon_partial_sums(d, F32, part_rows)
    ref64 = {**_per_graph("deg", d64), **_per_graph("part", p64)}
    ref32 = {**_per_graph("deg", d32), **_per_graph("part", p32)}
    zeros = {f"deg[{b}]": ~d["real"][b] for b in range(B)}
    fails = forward_errors(case, {**_per_graph("deg", deg), **_per_graph("part", part)}, ref64, ref32, zeros=zeros,
                           factor=factor_of("dmon"), report=report)
    assert torch.equal(part[:, :, 2 * Kc + 1].sum(1).cpu(), torch.tensor(d["n_b"], dtype=F32)), case  # the node counts
    if seed % 4 == 0:
        deg2, part2 = K.dmon_dense_terms(adj, s, mask, sizes)
        assert torch.equal(deg, deg2) and torch.equal(part, part2)
    if d["prefix"]:  # the un-padded layout of the same batch: both within the bound
        longest = max(d["n_b"])
        ptr = mv(d["ptr"])
        for in_deg in (False, True):
            de = K.dmon_edge_degrees(mv(d["edge_index"]), mv(d["edge_weight"]), ptr, mv(d["edge_ptr"]), longest, in_deg)
            want64 = (d["adj"].double().sum(1) if in_deg else d64)[:, :longest]
            want32 = (d["adj"].sum(1) if in_deg else d32)[:, :longest]
            fails += forward_errors(f"{case}-edge-degrees-{'in' if in_deg else 'out'}", _per_graph("deg", de),
                                    _per_graph("deg", want64), _per_graph("deg", want32),
                                    zeros={f"deg[{b}]": ~d["real"][b, :longest] for b in range(B)},
                                    factor=factor_of("dmon"), report=report)
        deg_flat = torch.cat([deg[b, :c] for b, c in enumerate(d["n_b"])])
        part_f = K.dmon_node_terms(mv(d["s_flat"]), deg_flat, ptr, longest)
        f64, f32 = FR.dmon_partial_sums(d, F64, part_rows, flat=True)[1], FR.dmon_partial_sums(d, F32, part_rows, flat=True)[1]
        assert tuple(part_f.shape) == tuple(f64.shape)
        fails += forward_errors(f"{case}-flat", _per_graph("part", part_f), _per_graph("part", f64),
                                _per_graph("part", f32), factor=factor_of("dmon"), report=report)
    # dS (+)= coef_0 deg ca + coef_1 cs: the backward's elementwise pass, padded and (prefix draws) un-padded
    ca, cs, coef = upstream(case + "ca", B, Kc), upstream(case + "cs", B, Kc), upstream(case + "coef", B, 2)
    old = upstream(case + "old", B, N, Kc) if seed % 2 else None
    out = mv(old).clone() if old is not None else torch.empty(B, N, Kc, device=dev())
    K.dmon_ds(deg, mv(ca), mv(cs), mv(coef), B * N, N, None, out, old is not None)

    def ds_ref(dtype):
        r = FR.dmon_ds_reference(deg.cpu(), ca, cs, coef, dtype)
        return r if old is None else r + old.to(dtype)
    fails += forward_errors(f"{case}-ds", _per_graph("dS", out), _per_graph("dS", ds_ref(F64)), _per_graph("dS", ds_ref(F32)),
                            factor=factor_of("dmon"), report=report)
    if d["prefix"]:
        rows = int(d["ptr"][-1])
        out_f = torch.empty(rows, Kc, device=dev())
        K.dmon_ds(deg_flat, mv(ca), mv(cs), mv(coef), rows, max(rows, 1), mv(d["batch"]), out_f, False)
        pick = lambda t: torch.cat([t[b, :c] for b, c in enumerate(d["n_b"])])  # noqa: E731
        fails += forward_errors(f"{case}-ds-flat", {"dS": out_f}, {"dS": pick(FR.dmon_ds_reference(deg.cpu(), ca, cs, coef, F64))},
                                {"dS": pick(FR.dmon_ds_reference(deg.cpu(), ca, cs, coef, F32))},
                                factor=factor_of("dmon"), report=report)
    finish(case, fails, report)


@pytest.mark.parametrize("seed", SEEDS)
def test_dmon_public(seed):
    from tgp.utils.losses import dmon_loss_terms
    d = FI.draw("dmon", seed, limits())
    case, report = f"dmon-public-{seed}", []
    fin = FR.dmon_finite(d)
    names = ("spectral", "cluster", "ortho")

    def run(graphs):
        s = mv(d["s"][graphs]).requires_grad_(True)
        adj = mv(d["adj"][graphs])
        raw = torch.matmul(torch.matmul(s.detach().transpose(1, 2), adj), s.detach()).requires_grad_(True)
        terms = dmon_loss_terms(adj, s, raw, None if d["mask"] is None else mv(d["mask"][graphs]),
                                None if d["graph_sizes"] is None else mv(d["graph_sizes"][graphs]))
        assert tuple(terms.shape) == (3, len(graphs)) and "_DMoNTermsFnBackward" in _graph_names(terms.grad_fn)
        return terms, s, raw
    every = list(range(d["B"]))
    terms, _, raw_all = run(every)  # values: the whole batch, the graph without a node in its place
    raw_all = raw_all.detach().cpu()
    got = {f"{n}[{b}]": terms[i, b] for i, n in enumerate(names) for b in fin}
    with torch.no_grad():
        fails = forward_errors(case, got, FR.dmon_reference(d, F64, raw_all)[0], FR.dmon_reference(d, F32, raw_all)[0],
                               factor=factor_of("dmon"), report=report)
    finish(case, fails, report)
    if not fin:
        return
    wanted = set(FR.dmon_reference(d, F64, raw_all, grads=True)[0])

    def kernel():  # gradients: the graphs with a real node (the others are 0 / 0 in every form)
        t, s, raw = run(fin)
        outs = {f"{n}[{b}]": t[i, j] for i, n in enumerate(names) for j, b in enumerate(fin)}
        return {n: v for n, v in outs.items() if n in wanted}, {"s": s, "raw": raw}
    check_grads(case, kernel, lambda dt: FR.dmon_reference(d, dt, raw_all, grads=True), ["s", "raw"])
    if seed % 4 == 0:
        runs = []
        for _ in range(2):
            t, s, raw = run(fin)
            runs.append([t.detach()] + list(torch.autograd.grad(t.sum(), [s, raw])))
        assert all(torch.equal(u, v) for u, v in zip(*runs)), case


# =========================================================================================================== LaPool
def _lapool_x(d):
    x = mv(d["x"])
    return offset_by_one_element(x) if d["layout"] == "edges_offset" else x


def _lapool_lead(d, v):
    """``K.lapool_leaders`` on the variations ``v`` (device) in the drawn layout."""
    from tgp import kernels as K
    if d["padded"]:
        return K.lapool_leaders(v, mv(d["adj"]), mv(d["mask"]))
    return K.lapool_leaders(v, edge_index=mv(d["edge_index"]), batch=mv(d["batch"]), ptr=mv(d["ptr"]))


def _lapool_check_leaders(case, d, lead, v_host):
    """Leader flags, columns and counts for the float32 variations as given: exact."""
    flags = FR.lapool_leaders(d, v_host)
    want = {"flags": flags.reshape(-1), **FR.lapool_columns(d, flags)}
    real = d["real"].reshape(-1) if d["padded"] else torch.ones(flags.numel(), dtype=torch.bool)
    got = {"flags": lead.flags.reshape(-1).cpu() & real, "col_of": torch.where(real, lead.col_of.cpu().long(), -1),
           "k": lead.k.cpu()}
    want["col_of"] = torch.where(real, want["col_of"], -1)
    assert lead.k_max == int(want["k"].max()), case
    return forward_errors(case, got, want, want, exact=set(want)), flags


@pytest.mark.parametrize("seed", SEEDS)
def test_lapool_operators(seed):
    """``lapool_variation`` against float64; ``lapool_leaders`` (flags, columns, counts: exact) on the kernel's own
    variations and on integer-valued ones full of ties; ``lapool_assign`` and its native backward for those leaders."""
    from tgp import kernels as K
    d = FI.draw("lapool", seed, limits())
    case, report = f"lapool-op-{seed}", []
    x = _lapool_x(d)
    B = len(d["n_b"])
    if d["padded"]:
        v = K.lapool_variation(x, mv(d["adj"]), mv(d["mask"]))
    else:
        ei = mv(d["edge_index"])
        by_src = K.lapool_edge_group(ei, d["n"])
        ascending = bool((d["edge_index"][0, 1:] >= d["edge_index"][0, :-1]).all())
        assert (by_src.perm is None) == (ascending and ei.size(1) > 0), case  # sorted sources: the CSR offsets alone
        v = K.lapool_variation(x, edge_index=ei, edge_weight=mv(d["edge_weight"]), by_src=by_src)
    rows = lambda t, b: FR.lapool_graph_rows(d, t, b)  # noqa: E731
    every = range(B)
    fails = forward_errors(case, {f"v[{b}]": rows(v, b) for b in every},
                           {f"v[{b}]": rows(FR.lapool_variation(d, F64), b) for b in every},
                           {f"v[{b}]": rows(FR.lapool_variation(d, F32), b) for b in every},
                           zeros={f"v[{b}]": ~d["real"][b] for b in every} if d["padded"] else None,
                           factor=factor_of("lapool"), report=report)
    more, _ = _lapool_check_leaders(f"{case}-tied", d, _lapool_lead(d, mv(d["v_tied"])), d["v_tied"])
    fails += more
    lead = _lapool_lead(d, v)
    more, flags = _lapool_check_leaders(f"{case}-own", d, lead, v.cpu())
    fails += more
    s, nrm = K.lapool_assign(x, lead)
    r64, r32 = FR.lapool_reference(d, F64, flags)[0], FR.lapool_reference(d, F32, flags)[0]
    kmax = lead.k_max
    ks = FR.lapool_columns(d, flags)["k"]
    zeros = {}
    for b in every:  # padded rows and the columns from k_b on: exact zeros
        z = torch.zeros(rows(s, b).shape, dtype=torch.bool)
        z[:, int(ks[b]):] = True
        if d["padded"]:
            z[~d["real"][b]] = True
        zeros[f"S[{b}]"] = z
    with torch.no_grad():
        fails += forward_errors(f"{case}-assign", {f"S[{b}]": rows(s, b) for b in every}, r64, r32, zeros=zeros,
                                factor=factor_of("lapool"), report=report)
    nrm64 = d["x"].double().norm(dim=-1).reshape(-1)
    real = d["real"].reshape(-1) if d["padded"] else torch.ones(nrm64.numel(), dtype=torch.bool)
    fails += forward_errors(f"{case}-assign", {"nrm": nrm.cpu()[real]}, {"nrm": nrm64[real]},
                            {"nrm": d["x"].norm(dim=-1).reshape(-1)[real]}, factor=factor_of("lapool"), report=report)
    if kmax > 0:  # the native backward operator on one upstream gradient
        ds = upstream(case, *s.shape)
        dx = K.lapool_assign_bwd(x, nrm, s, mv(ds), lead)

        def ref_dx(dtype):
            outs, lv = FR.lapool_reference(d, dtype, flags)
            total = sum((outs[f"S[{b}]"] * rows(ds, b).to(dtype)).sum() for b in every)
            (gx,) = torch.autograd.grad(total, lv["x"])
            return {f"dx[{b}]": rows(gx, b) for b in every}
        zx = {f"dx[{b}]": (~d["real"][b]).unsqueeze(-1).expand(-1, d["F"]) for b in every} if d["padded"] else None
        fails += forward_errors(f"{case}-bwd", {f"dx[{b}]": rows(dx, b) for b in every}, ref_dx(F64), ref_dx(F32),
                                zeros=zx, factor=factor_of("lapool"), report=report)
        if seed % 4 == 0:
            s2, nrm2 = K.lapool_assign(x, lead)
            assert torch.equal(s, s2) and torch.equal(nrm, nrm2)
            assert torch.equal(K.lapool_assign_bwd(x, nrm, s, mv(ds), lead), dx), case
    finish(case, fails, report)


@pytest.mark.parametrize("seed", SEEDS)
def test_lapool_public(seed):
    """``functions.lapool_assign`` (one autograd node, the native backward) per graph, gradients to x one graph at a
    time, for the leaders of the integer-valued variations (fixed, exact: no float decides the leader set)."""
    from tgp import functions as Fn
    d = FI.draw("lapool", seed, limits())
    case, report = f"lapool-public-{seed}", []
    lead = _lapool_lead(d, mv(d["v_tied"]))
    flags = FR.lapool_leaders(d, d["v_tied"])
    assert torch.equal(lead.k.cpu().long(), FR.lapool_columns(d, flags)["k"]), case
    B = len(d["n_b"])

    def kernel():
        x = _lapool_x(d).detach().requires_grad_(True)
        s = Fn.lapool_assign(x, lead)
        assert "_LaPoolAssignFnBackward" in _graph_names(s.grad_fn)
        return {f"S[{b}]": FR.lapool_graph_rows(d, s, b) for b in range(B)}, {"x": x}
    outs, _ = kernel()
    with torch.no_grad():
        fails = forward_errors(case, outs, FR.lapool_reference(d, F64, flags)[0], FR.lapool_reference(d, F32, flags)[0],
                               factor=factor_of("lapool"), report=report)
    finish(case, fails, report)
    if lead.k_max > 0:
        check_grads(case, kernel, lambda dt: FR.lapool_reference(d, dt, flags), ["x"])


# =================================================================================================== AsymCheegerCut
def _acc_quantile_checks(case, d, got, want, graphs, small, route, fails, report, colsum_of):
    """One ``acc_quantile`` result against the exact selection (value, LOWEST row that holds it, rows >= it, real rows)
    on the graphs with a real node, its route, and the asymmetric-norm column sums."""
    q, qnode, colsum, cge, nreal, taken = got
    assert taken == ("count" if route == "count" or (route == "auto" and small) else "radix"), (case, route, taken)
    have = {"q": q.cpu()[graphs], "qnode": qnode.cpu()[graphs], "cge": cge.cpu()[graphs], "nreal": nreal.cpu()}
    ref = {n: (v if n == "nreal" else v[graphs]) for n, v in want.items()}
    fails += forward_errors(f"{case}-{route}", have, ref, ref, exact=set(ref))
    fails += forward_errors(f"{case}-{route}", {"colsum": colsum.cpu()[graphs]}, {"colsum": colsum_of(F64)[graphs]},
                            {"colsum": colsum_of(F32)[graphs]}, factor=factor_of("acc"), report=report)


@pytest.mark.parametrize("seed", SEEDS)
def test_acc_operators(seed):
    """The total variation (dense blocks of 16 rows; per node over the listed edges), the quantile select on both routes
    where the size permits, the tail, and the three native backward operators on one upstream gradient each -- padded
    and, where the real rows are a prefix, un-padded with its hub."""
    from tgp import kernels as K
    lim = limits()
    d = FI.draw("acc", seed, lim)
    case, report = f"acc-op-{seed}", []
    s, adj, mask, sizes = mv(d["s"]), mv(d["adj"]), mv(d["mask"]), mv(d["graph_sizes"])
    B, N, Kc = d["s"].shape
    k, fin = d["loss_k"], FR.dmon_finite(d)
    every = list(range(B))
    # ---- padded: forward
    part, cnt = K.acc_tv_dense(adj, s, sizes)
    (p64, c64), (p32, _) = FR.acc_tv_blocks(d, F64, lim["acc_tv_rows"]), FR.acc_tv_blocks(d, F32, lim["acc_tv_rows"])
    assert tuple(part.shape) == tuple(p64.shape) and torch.equal(cnt.cpu().long(), c64), case
    fails = forward_errors(f"{case}-tv", _per_graph("part", part), _per_graph("part", p64), _per_graph("part", p32),
                           factor=factor_of("acc"), report=report)
    small = N <= lim["acc_small_graph_nodes"]
    assert small == (N <= K.acc_small_graph_nodes())
    want = FR.acc_quantile_exact(d)
    colsum_of = lambda dt: FR.acc_colsum(d, dt, want["q"])  # noqa: E731
    sel = None  # (k <= 1: no balance term -- the select and its backward are not run, as the loss Function has it)
    for route in (["auto"] + (["count", "radix"] if small else [])) if k > 1 else []:  # (auto beyond the limit: radix)
        got = K.acc_quantile(s, k, mask=mask, graph_sizes=sizes, route=route)
        _acc_quantile_checks(case, d, got, want, fin, small, route, fails, report, colsum_of)
        sel = got if sel is None else sel
    q, qnode, colsum, cge, nreal, _ = sel if sel is not None else (None,) * 6
    out, ecnt = K.acc_tail(B, Kc, k, dev(), ("dense", part, cnt), colsum, nreal)
    assert torch.equal(ecnt.cpu().long().clamp(min=1), c64.sum(1).clamp(min=1)), case
    r64, r32 = FR.acc_reference(d, F64)[0], FR.acc_reference(d, F32)[0]
    with torch.no_grad():
        fails += forward_errors(f"{case}-tail", {**_per_graph("tv", out[0]), **_per_graph("balance", out[1])}, r64, r32,
                                factor=factor_of("acc"), report=report)
    # ---- padded: the native backward operators
    g = upstream(case, 2, B)
    old = upstream(case + "old", B, N, Kc) if seed % 2 else None
    d_tv = K.acc_tv_dense_bwd(adj, s, sizes, mv(g[0]), ecnt, 1.0)
    d_bal = mv(old).clone() if old is not None else torch.zeros(B, N, Kc, device=dev())
    if k > 1:
        K.acc_asym_bwd(s, k, q, qnode, cge, nreal, mv(g[1]), 1.0, d_bal, old is not None, mask=mask, graph_sizes=sizes)

    def ref_grads(dtype, reference=FR.acc_reference, rows=lambda t, b: t[b], graphs=every, prior=old):
        outs, lv = reference(d, dtype)
        res = {}
        for i, name in enumerate(("tv", "balance")):
            total = sum(g[i, b].to(dtype) * outs[f"{name}[{b}]"] for b in graphs)
            gs = torch.autograd.grad(total, lv["s"], allow_unused=True)[0] if total.requires_grad else None
            gs = torch.zeros_like(lv["s"]) if gs is None else gs
            if name == "balance" and prior is not None:
                gs = gs + prior.to(dtype)
            res.update({f"d_{name}[{b}]": rows(gs, b) for b in graphs})
        return res
    got = {**_per_graph("d_tv", d_tv), **_per_graph("d_balance", d_bal)}
    zeros = None if old is not None else {f"d_balance[{b}]": (~d["real"][b]).unsqueeze(-1).expand(-1, Kc) for b in every}
    fails += forward_errors(f"{case}-bwd", got, ref_grads(F64), ref_grads(F32), zeros=zeros, factor=factor_of("acc"),
                            report=report)
    if seed % 4 == 0:
        assert all(torch.equal(u, v) for u, v in zip(K.acc_tv_dense(adj, s, sizes), (part, cnt)))
        if k > 1:
            assert all(torch.equal(u, v) for u, v in zip(K.acc_quantile(s, k, mask=mask, graph_sizes=sizes)[:5], sel[:5]))
        assert torch.equal(K.acc_tv_dense_bwd(adj, s, sizes, mv(g[0]), ecnt, 1.0), d_tv)
    # ---- un-padded: the same batch as rows with ptr and an edge list (duplicates, the hub)
    if d["prefix"]:
        sf, ei, w = mv(d["s_flat"]), mv(d["edge_index"]), mv(d["edge_weight"])
        ptr, batch, n = mv(d["ptr"]), mv(d["batch"]), d["n"]
        by_src, by_dst = K.edge_group(ei, n), K.edge_group(ei, n, by_destination=True)
        node_tv = K.acc_tv_edge(sf, ei, w, by_src)
        fails += forward_errors(f"{case}-edge-tv", {"node_tv": node_tv}, {"node_tv": FR.acc_node_tv(d, F64)},
                                {"node_tv": FR.acc_node_tv(d, F32)}, factor=factor_of("acc"), report=report)
        longest = max(d["n_b"])
        fsmall = longest <= lim["acc_small_graph_nodes"]
        fsel = None
        for route in (["auto"] + (["count", "radix"] if fsmall else [])) if k > 1 else []:
            got = K.acc_quantile(sf, k, ptr=ptr, max_nodes=longest, route=route)
            _acc_quantile_checks(f"{case}-flat", d, got, want, fin, fsmall, route, fails, report, colsum_of)
            fsel = got if fsel is None else fsel
        fsel = fsel if fsel is not None else (None,) * 6
        fout, fecnt = K.acc_tail(B, Kc, k, dev(), ("edge", node_tv, by_src, ptr), fsel[2], fsel[4])
        edges = torch.bincount(d["batch"][d["edge_index"][0]], minlength=B)
        assert torch.equal(fecnt.cpu().long().clamp(min=1), edges.clamp(min=1)), case
        f64, f32 = FR.acc_flat_reference(d, F64)[0], FR.acc_flat_reference(d, F32)[0]
        with torch.no_grad():
            fails += forward_errors(f"{case}-flat-tail", {**_per_graph("tv", fout[0]), **_per_graph("balance", fout[1])},
                                    f64, f32, factor=factor_of("acc"), report=report)
        e_tv = K.acc_tv_edge_bwd(sf, ei, w, by_src, by_dst, batch, mv(g[0]), fecnt, 1.0)
        e_bal = torch.zeros(n, Kc, device=dev())
        if k > 1:
            K.acc_asym_bwd(sf, k, fsel[0], fsel[1], fsel[3], fsel[4], mv(g[1]), 1.0, e_bal, False, ptr=ptr, batch=batch)
        seg = lambda t, b: t[int(d["ptr"][b]):int(d["ptr"][b + 1])]  # noqa: E731
        got = {f"d_tv[{b}]": seg(e_tv, b) for b in every}
        got.update({f"d_balance[{b}]": seg(e_bal, b) for b in every})
        flat = dict(reference=FR.acc_flat_reference, rows=seg, prior=None)
        # (a hub's edges cross the rows of its graph only: every graph's rows still depend on its own term alone)
        fails += forward_errors(f"{case}-flat-bwd", got, ref_grads(F64, **flat), ref_grads(F32, **flat),
                                factor=factor_of("acc"), report=report)
    finish(case, fails, report)


@pytest.mark.parametrize("seed", SEEDS)
def test_acc_public(seed):
    from tgp.utils.losses import acc_loss_terms, acc_sparse_loss_terms
    d = FI.draw("acc", seed, limits())
    case, report = f"acc-public-{seed}", []
    B, k = d["B"], d["loss_k"]
    adj, mask, sizes = mv(d["adj"]), mv(d["mask"]), mv(d["graph_sizes"])

    def kernel():
        s = mv(d["s"]).requires_grad_(True)
        terms = acc_loss_terms(adj, s, k, mask, sizes)
        assert tuple(terms.shape) == (2, B) and "_ACCTermsFnBackward" in _graph_names(terms.grad_fn)
        return {**_per_graph("tv", terms[0]), **_per_graph("balance", terms[1])}, {"s": s}
    outs, _ = kernel()
    with torch.no_grad():
        fails = forward_errors(case, outs, FR.acc_reference(d, F64)[0], FR.acc_reference(d, F32)[0],
                               factor=factor_of("acc"), report=report)
    runs = [(kernel, lambda dt: FR.acc_reference(d, dt), case)]
    if d["prefix"]:  # the un-padded public form of the same batch (graphs up to the last one with a node)
        ei, w, batch = mv(d["edge_index"]), mv(d["edge_weight"]), mv(d["batch"])
        nb = int(d["batch"].max()) + 1

        def trimmed(dt):
            o, lv = FR.acc_flat_reference(d, dt)
            return {n: v for n, v in o.items() if int(n[n.index("[") + 1:-1]) < nb}, lv

        def kernel_flat():
            s = mv(d["s_flat"]).requires_grad_(True)
            terms = acc_sparse_loss_terms(ei, w, s, k, batch)
            assert terms is not None and tuple(terms.shape) == (2, nb)
            assert "_ACCTermsFnBackward" in _graph_names(terms.grad_fn)
            return {**_per_graph("tv", terms[0]), **_per_graph("balance", terms[1])}, {"s": s}
        flat_outs = kernel_flat()[0]
        with torch.no_grad():
            fails += forward_errors(f"{case}-flat", flat_outs, trimmed(F64)[0], trimmed(F32)[0],
                                    factor=factor_of("acc"), report=report)
        runs.append((kernel_flat, trimmed, f"{case}-flat"))
    finish(case, fails, report)
    for run, oracle, name in runs:
        check_grads(name, run, oracle, ["s"])
        if seed % 4 == 0:
            twice = []
            for _ in range(2):
                o, lv = run()
                twice.append([torch.stack(list(o.values())).detach(), torch.autograd.grad(sum(o.values()), lv["s"])[0]])
            assert all(torch.equal(u, v) for u, v in zip(*twice)), name


# ============================================================================================================= HOSC
@pytest.mark.parametrize("seed", SEEDS)
def test_hosc_operators(seed):
    """The motif chain without A A A: three ``hosc_matvec`` passes and three products (general route) and, where the
    batch fits it, the one-launch ``hosc_small``: d1 = A 1, d3 = A A A 1, z = A A A S against the explicit cube."""
    from tgp import kernels as K
    lim = limits()
    d = FI.draw("hosc", seed, lim)
    case, report = f"hosc-op-{seed}", []
    s, adj, mask, sizes = mv(d["s"]), mv(d["adj"]), mv(d["mask"]), mv(d["graph_sizes"])
    B, N, Kc = d["s"].shape
    small = K.hosc_is_small(N, Kc)
    assert small == (N <= lim["hosc_small_graph_nodes"] and Kc <= lim["hosc_small_graph_nodes"]), case
    names = ("d1", "d3", "z")
    r64 = {f"{n}[{b}]": t[b] for n, t in zip(names, FR.hosc_chain(d, F64)) for b in range(B)}
    r32 = {f"{n}[{b}]": t[b] for n, t in zip(names, FR.hosc_chain(d, F32)) for b in range(B)}
    zeros = {f"{n}[{b}]": (~d["real"][b]).unsqueeze(-1).expand(-1, Kc) if n == "z" else ~d["real"][b]
             for n in names for b in range(B)}
    d1 = K.hosc_matvec(adj, None, sizes)
    d3 = K.hosc_matvec(adj, K.hosc_matvec(adj, d1, sizes), sizes)
    z = K.bmm(adj, K.bmm(adj, K.bmm(adj, s)))
    got = {f"{n}[{b}]": t[b] for n, t in zip(names, (d1, d3, z)) for b in range(B)}
    fails = forward_errors(f"{case}-chain", got, r64, r32, zeros=zeros, factor=factor_of("hosc"), report=report)
    if small:
        zs, d1s, d3s, part = K.hosc_small(adj, s, mask, sizes)
        assert tuple(part.shape) == (B, 1, int(K.N.lib().tgp_hosc_record_floats(Kc)))
        got = {f"{n}[{b}]": t[b] for n, t in zip(names, (d1s, d3s, zs)) for b in range(B)}
        fails += forward_errors(f"{case}-small", got, r64, r32, zeros=zeros, factor=factor_of("hosc"), report=report)
        if seed % 4 == 0:
            again = K.hosc_small(adj, s, mask, sizes)
            assert all(torch.equal(u, v) for u, v in zip((zs, d1s, d3s, part), again)), case
        # the one-launch record (its num1 = sum S (.) A S comes from the first round) and hosc_node_terms on the general
        # route's operands, with and without that first product: the same records
        z1 = K.bmm(adj, s)

        def chain_record(dt, with_z1):
            c1, c3, cz = FR.hosc_chain(d, dt)
            cz1 = d["adj"].to(dt) @ d["s"].to(dt) if with_z1 else torch.zeros_like(cz)
            return FR.hosc_records(d, dt, cz, cz1, c3, c1, lim["part_rows"])
        for name, have, with_z1 in (("small", part, True), ("general", K.hosc_node_terms(s, z, None, d3, d1, mask, sizes), False),
                                    ("general-z1", K.hosc_node_terms(s, z, z1, d3, d1, mask, sizes), True)):
            fails += forward_errors(f"{case}-record-{name}", _per_graph("part", have),
                                    _per_graph("part", chain_record(F64, with_z1)),
                                    _per_graph("part", chain_record(F32, with_z1)), factor=factor_of("hosc"), report=report)
    # hosc_node_terms and the backward's elementwise hosc_ds on operands of their own, every term switched on
    zr, z1r, ztr, z1tr = (upstream(case + n, B, N, Kc) for n in ("z", "z1", "zt", "z1t"))
    d3r, d1r = upstream(case + "d3", B, N).abs(), upstream(case + "d1", B, N).abs()
    part_r = K.hosc_node_terms(s, mv(zr), mv(z1r), mv(d3r), mv(d1r), mask, sizes)
    assert tuple(part_r.shape) == (B, max(1, -(-N // lim["part_rows"])), int(K.N.lib().tgp_hosc_record_floats(Kc)))
    rec = lambda dt: FR.hosc_records(d, dt, zr, z1r, d3r, d1r, lim["part_rows"])  # noqa: E731
    fails += forward_errors(f"{case}-node-terms", _per_graph("part", part_r), _per_graph("part", rec(F64)),
                            _per_graph("part", rec(F32)), factor=factor_of("hosc"), report=report)
    cn, coef = upstream(case + "cn", B, Kc).abs() + 0.5, upstream(case + "coef", B, 5)
    old = upstream(case + "old", B, N, Kc) if seed % 2 else None
    out = mv(old).clone() if old is not None else torch.empty(B, N, Kc, device=dev())
    K.hosc_ds(s, mv(zr), mv(ztr), mv(z1r), mv(z1tr), mv(d3r), mv(d1r), mv(cn), mv(coef), N, None, out, old is not None)

    def ds_ref(dt):
        r = FR.hosc_ds_reference(d, dt, zr, ztr, z1r, z1tr, d3r, d1r, cn, coef)
        return r if old is None else r + old.to(dt)
    fails += forward_errors(f"{case}-ds", _per_graph("dS", out), _per_graph("dS", ds_ref(F64)), _per_graph("dS", ds_ref(F32)),
                            factor=factor_of("hosc"), report=report)
    finish(case, fails, report)


@pytest.mark.parametrize("seed", SEEDS)
def test_hosc_public(seed):
    from tgp import kernels as K
    from tgp.utils.losses import hosc_loss_terms
    lim = limits()
    d = FI.draw("hosc", seed, lim)
    case, report = f"hosc-public-{seed}", []
    fin = FR.dmon_finite(d)
    small = d["N"] <= lim["hosc_small_graph_nodes"] and d["K"] <= lim["hosc_small_graph_nodes"]
    assert K.hosc_is_small(d["N"], d["K"]) == small, case  # the route the draw was made to reach
    use_raw = d["with_raw"] and d["alpha"] < 1

    def run(graphs):
        s = mv(d["s"][graphs]).requires_grad_(True)
        adj = mv(d["adj"][graphs])
        raw = None
        if d["with_raw"]:
            raw = torch.matmul(torch.matmul(s.detach().transpose(1, 2), adj), s.detach()).requires_grad_(True)
        terms = hosc_loss_terms(adj, s, raw, None if d["mask"] is None else mv(d["mask"][graphs]),
                                None if d["graph_sizes"] is None else mv(d["graph_sizes"][graphs]),
                                alpha=d["alpha"], mu=d["mu"], hosc_ortho=d["hosc_ortho"])
        assert tuple(terms.shape) == (2, len(graphs)) and "_HOSCTermsFnBackward" in _graph_names(terms.grad_fn)
        return terms, s, raw
    terms, _, raw_all = run(list(range(d["B"])))  # values: the whole batch, the graph without a node in its place
    raw_all = raw_all.detach().cpu() if use_raw else None
    got = {f"{n}[{b}]": terms[i, b] for i, n in enumerate(("hosc", "ortho")) for b in fin}
    with torch.no_grad():
        fails = forward_errors(case, got, FR.hosc_reference(d, F64, raw_all)[0], FR.hosc_reference(d, F32, raw_all)[0],
                               factor=factor_of("hosc"), report=report)
    finish(case, fails, report)
    if not fin:
        return
    wanted = set(FR.hosc_reference(d, F64, raw_all, grads=True)[0])

    def kernel():  # gradients: the graphs with a real node (the others are 0 / 0 in every form)
        t, s, raw = run(fin)
        outs = {f"{n}[{b}]": t[i, j] for i, n in enumerate(("hosc", "ortho")) for j, b in enumerate(fin)}
        return {n: v for n, v in outs.items() if n in wanted}, {"s": s, "raw": raw if use_raw else None}
    check_grads(case, kernel, lambda dt: FR.hosc_reference(d, dt, raw_all, grads=True), ["s", "raw"])
    if seed % 4 == 0:
        runs = []
        for _ in range(2):
            t, s, _ = run(fin)
            runs.append([t.detach(), torch.autograd.grad(t.sum(), s)[0]])
        assert all(torch.equal(u, v) for u, v in zip(*runs)), case


# ========================================================================================================== BN-Pool
def _bnpool_rows(d, t):
    """Per graph with a real node: the rows of a [B,N,K] tensor; the rows outside the mask must be exact zeros."""
    return {b: t[b] for b in FR.bnpool_finite(d)}


@pytest.mark.parametrize("seed", SEEDS)
def test_bnpool_operators(seed):
    from tgp import kernels as K
    d = FI.draw("bnpool", seed, limits())
    case, report = f"bnpool-op-{seed}", []
    assert d["K"] <= K.bnpool_max_clusters()
    s, adj, mask = mv(d["s"]), mv(d["adj"]), mv(d["mask"])
    t = torch.matmul(s, mv(d["k_mat"]))
    rec, stats = K.bnpool_rec_fwd(t, s, adj, mask)
    assert rec.dtype == F32 and tuple(rec.shape) == (d["B"],) and tuple(stats.shape) == (d["B"], 2)
    fin = FR.bnpool_finite(d)

    def reference(dtype):  # (T as the device formed it: the operators are judged on their own inputs)
        return FR.bnpool_operator_reference(d, dtype, t=t.cpu())
    r64, r32 = reference(F64)[0], reference(F32)[0]
    fails = forward_errors(case, {f"rec[{b}]": rec[b] for b in fin}, r64, r32, factor=factor_of("bnpool"), report=report)
    n2 = torch.tensor([float(n * n) for n in d["n_b"]])
    assert torch.equal(stats[:, 1].cpu(), n2), case
    g = upstream(case, d["B"])
    g[[b for b in range(d["B"]) if b not in fin]] = 0
    p, q = K.bnpool_rec_bwd(t, s, adj, mask, mv(g), stats)

    def ref_grads(dtype):
        outs, lv = reference(dtype)
        if not outs:
            return {}
        total = sum(g[b].to(dtype) * outs[f"rec[{b}]"] for b in fin)
        gt, gs = torch.autograd.grad(total, [lv["t"], lv["s"]])
        out = {f"P[{b}]": gt[i] for i, b in enumerate(fin)}
        out.update({f"Q[{b}]": gs[i] for i, b in enumerate(fin)})
        return out
    got = {f"P[{b}]": p[b] for b in fin}
    got.update({f"Q[{b}]": q[b] for b in fin})
    outside = ~FR.bnpool_row_mask(d)
    zeros = {f"{w}[{b}]": outside[b].expand(-1, d["K"]) for w in "PQ" for b in fin}
    fails += forward_errors(case, got, ref_grads(F64), ref_grads(F32), zeros=zeros, factor=factor_of("bnpool"),
                            report=report)
    if seed % 4 == 0:
        rec2, stats2 = K.bnpool_rec_fwd(t, s, adj, mask)
        p2, q2 = K.bnpool_rec_bwd(t, s, adj, mask, mv(g), stats2)
        assert torch.equal(rec[fin], rec2[fin]) and torch.equal(stats, stats2)
        assert all(torch.equal(p[b], p2[b]) and torch.equal(q[b], q2[b]) for b in fin)
    finish(case, fails, report)


@pytest.mark.parametrize("seed", SEEDS)
def test_bnpool_public(seed):
    from tgp.utils.losses import bnpool_rec_loss_terms
    d = FI.draw("bnpool", seed, limits())
    case, report = f"bnpool-public-{seed}", []
    fin = FR.bnpool_finite(d)
    adj, mask = mv(d["adj"]), mv(d["mask"])

    def kernel(graphs=fin):
        """The public call on ``graphs`` (gradients: those with a real node; a graph without one is 0 / 0 in every
        form and would put NaN into the shared cluster matrix's gradient)."""
        s, k_mat = mv(d["s"][graphs]).requires_grad_(True), mv(d["k_mat"]).requires_grad_(True)
        rec = bnpool_rec_loss_terms(s, k_mat, adj[graphs], None if mask is None else mask[graphs])
        assert "_BNPoolRecFnBackward" in _graph_names(rec.grad_fn)  # the native route, never the composed form
        return {f"rec[{b}]": rec[i] for i, b in enumerate(graphs) if b in fin}, {"s": s, "k_mat": k_mat}
    outs, _ = kernel(list(range(d["B"])))  # values: the whole batch, the graph without a node in its place
    with torch.no_grad():
        fails = forward_errors(case, outs, FR.bnpool_reference(d, F64)[0], FR.bnpool_reference(d, F32)[0],
                               factor=factor_of("bnpool"), report=report)
    finish(case, fails, report)
    if fin:
        check_grads(case, kernel, lambda dt: FR.bnpool_reference(d, dt), ["s", "k_mat"])
    if seed % 4 == 0 and fin:  # the same public call twice: equal bits, forward and backward
        twice = []
        for _ in range(2):
            o, lv = kernel()
            twice.append([torch.stack(list(o.values())).detach()]
                         + list(torch.autograd.grad(sum(o.values()), [lv["s"], lv["k_mat"]])))
        assert all(torch.equal(u, v) for u, v in zip(*twice)), case


# ========================================================================================================== readout
def _readout_call(d, x, want_aux=True):
    """K.segment_aggr on the drawn row source: (out, ties, count, what the backward operator needs or None)."""
    from tgp import kernels as K
    ops_mask = K.segment_ops_mask(d["ops"])
    lay, g = d["layout"], d["groups"]
    if lay.startswith("ptr"):
        out = K.segment_aggr(x, ops_mask, g, d["max_len"], ptr=mv(d["ptr"]), want_aux=want_aux)
        return out, dict(batch=mv(d["batch"]))
    if lay.startswith("dense"):
        m = None if d["mask"] is None else mv(d["mask"]).reshape(-1).contiguous().view(torch.uint8)
        out = K.segment_aggr(x.reshape(-1, d["F"]), ops_mask, g, d["max_len"], dense_nodes=d["N"], mask=m,
                             want_aux=want_aux)
        return out, dict(dense_nodes=d["N"], mask=m)
    index = K.build_assign_index(mv(d["cluster_index"]), g)
    assert index.max_members == d["max_len"]
    out = K.segment_aggr(x, ops_mask, g, index.max_members, index=index, node_index=mv(d["node_index"]),
                         weight=mv(d["weight"]), want_aux=want_aux)
    return out, None


def _readout_x(d):
    if d["layout"] == "ptr_sliced":
        x = mv(d["x_base"])[:, d["first"]:d["first"] + d["F"]]
        assert x.stride(0) == d["F"] + 7
        return x
    x = mv(d["x"])
    if d["layout"].startswith("dense") and d["mask"] is not None:  # a masked row is never read
        x = torch.where(mv(d["mask"]).unsqueeze(-1), x, torch.full_like(x, float("nan")))
    return x


def _blocks(d, t, ops=None):
    ops = d["ops"] if ops is None else ops
    f = t.size(1) // len(ops)
    return {op: t[:, i * f:(i + 1) * f] for i, op in enumerate(ops)}


def _readout_exact_names(d):
    """max / min are selections among float32 values; integer-valued rows make every sum (and the one division of the
    mean) exact in float32: compared with ``torch.equal`` against the float32 restatement."""
    return set(d["ops"]) if d["integer"] else {op for op in d["ops"] if op in ("min", "max")}


@pytest.mark.parametrize("seed", SEEDS)
def test_readout_operators(seed):
    from tgp import kernels as K
    lim = limits()
    d = FI.draw("readout", seed, lim)
    case, report = f"readout-op-{seed}", []
    x = _readout_x(d)
    ops_mask = K.segment_ops_mask(d["ops"])
    # the route: a segment longer than one chunk sends the batch to the split route, which alone needs a workspace
    split = d["max_len"] > K.segment_aggr_chunk_rows()
    wsb = K.N.lib().tgp_segment_aggr_workspace_bytes(d["groups"], d["F"], ops_mask, d["max_len"])
    assert (wsb > 0) == split and split == (d["max_len"] > lim["segment_chunk_rows"]), (case, wsb, d["max_len"])
    (out, ties, count), bwd = _readout_call(d, x)
    r64, r32 = FR.readout_reference(d, F64)[0], FR.readout_reference(d, F32)[0]
    with torch.no_grad():
        fails = forward_errors(case, _blocks(d, out), r64, r32, exact=_readout_exact_names(d), exact_ref=r32,
                               factor=factor_of("readout"), report=report)
    want = FR.readout_exact(d)
    assert torch.equal(count.cpu().long(), want["count"]), case
    some = want["count"] > 0  # (the tie count of a group without rows is never read)
    mm = [op for op in d["ops"] if op in ("min", "max")]
    for op, blk in (_blocks(d, ties, mm).items() if mm else ()):
        assert torch.equal(blk.cpu().long()[some], want[f"ties_{op}"][some]), (case, op)
    assert bool((out[~mv(some)] == 0).all()), case  # groups without rows give 0 for every operation
    out_plain = _readout_call(d, x, want_aux=False)[0][0]
    assert torch.equal(out_plain, out)
    if bwd is not None:  # the native backward operator (contiguous and dense sources) on one upstream gradient
        g = upstream(case, *out.shape)
        x2 = x.reshape(-1, d["F"])
        dx = K.segment_aggr_bwd(mv(g), x2, out, ties, count, ops_mask, d["groups"], **bwd)

        def ref_grad(dtype):
            outs, lv = FR.readout_reference(d, dtype)
            y = torch.cat([outs[op] for op in d["ops"]], -1)
            return {"dx": torch.autograd.grad(y, lv["x"], g.to(dtype))[0].reshape(-1, d["F"])}
        zeros = None
        if d["layout"].startswith("dense") and d["mask"] is not None:
            zeros = {"dx": ~d["mask"].reshape(-1, 1).expand(-1, d["F"])}
        fails += forward_errors(case, {"dx": dx}, ref_grad(F64), ref_grad(F32), zeros=zeros,
                                factor=factor_of("readout"), report=report)
        if seed % 4 == 0:
            assert torch.equal(dx, K.segment_aggr_bwd(mv(g), x2, out, ties, count, ops_mask, d["groups"], **bwd))
    if seed % 4 == 0:
        again = _readout_call(d, x)[0]
        assert torch.equal(out, again[0]) and torch.equal(count, again[2])
        assert ties is None or torch.equal(ties, again[1])
        # the same groups through all three row sources (contiguous, dense with a mask, gathered): each within the bound
        for name, got in _readout_three_sources(d).items():
            with torch.no_grad():
                fails += forward_errors(f"{case}-as-{name}", _blocks(d, got), r64, r32, exact=_readout_exact_names(d),
                                        exact_ref=r32, factor=factor_of("readout"), report=report)
    finish(case, fails, report)


def _readout_three_sources(d):
    """The draw's groups (its float32 rows, weighted where it has weights) handed to ``K.segment_aggr`` as contiguous
    segments, as a padded batch with a prefix mask and as a gathered assignment: {source: out}."""
    from tgp import kernels as K
    rows = FR.readout_rows(d, d["x"], d.get("weight"))
    index, g, f = d["index"], d["groups"], d["F"]
    ops_mask = K.segment_ops_mask(d["ops"])
    order = torch.argsort(index, stable=True)
    counts = torch.bincount(index, minlength=g)
    ptr = torch.zeros(g + 1, dtype=torch.long)
    ptr[1:] = counts.cumsum(0)
    longest = int(counts.max())
    out = {"ptr": K.segment_aggr(mv(rows[order].contiguous()), ops_mask, g, longest, ptr=mv(ptr))[0]}
    width = max(longest, 1)
    padded = torch.full((g, width, f), float("nan"))  # (a masked row is never read)
    mask = torch.arange(width).view(1, -1) < counts.view(-1, 1)
    padded[mask] = rows[order]
    out["dense"] = K.segment_aggr(mv(padded.reshape(-1, f)), ops_mask, g, width, dense_nodes=width,
                                  mask=mv(mask).reshape(-1).contiguous().view(torch.uint8))[0]
    assign = K.build_assign_index(mv(index), g)
    out["gather"] = K.segment_aggr(mv(rows.contiguous()), ops_mask, g, assign.max_members, index=assign,
                                   node_index=mv(torch.arange(rows.size(0))))[0]
    return out


def _readout_public(d, x, weight=None):
    from tgp.reduce import AggrReduce, GlobalReduce, get_aggr
    from tgp.select import SelectOutput
    ops = list(d["ops"])
    op, kw = ("multi", {"aggrs": ops}) if len(ops) > 1 else (ops[0], {})
    lay = d["layout"]
    if lay.startswith("ptr"):
        return GlobalReduce(op, **kw)(x, batch=mv(d["batch"]), size=d["groups"])
    if lay.startswith("dense"):
        return GlobalReduce(op, **kw)(x, mask=mv(d["mask"]))
    so = SelectOutput(node_index=mv(d["node_index"]), cluster_index=mv(d["cluster_index"]),
                      weight=None if weight is None else weight.detach(), num_nodes=d["num_nodes"],
                      num_supernodes=d["groups"])
    if weight is not None:
        so._hold_values(weight)
    return AggrReduce(get_aggr(op, **kw))(x, so)[0]


@pytest.mark.parametrize("seed", SEEDS)
def test_readout_public(seed):
    d = FI.draw("readout", seed, limits())
    case, report = f"readout-public-{seed}", []

    def kernel():
        x = _readout_x(d).detach().requires_grad_(True)  # (a column slice stays a view with its own row stride)
        w = None if d.get("weight") is None else mv(d["weight"]).requires_grad_(True)
        out = _readout_public(d, x, w)
        assert out.dtype == F32 and "_SegmentAggrFnBackward" in _graph_names(out.grad_fn)
        return _blocks(d, out), {"x": x, "weight": w}

    outs, _ = kernel()
    r64, r32 = FR.readout_reference(d, F64)[0], FR.readout_reference(d, F32)[0]
    with torch.no_grad():
        fails = forward_errors(case, outs, r64, r32, exact=_readout_exact_names(d), exact_ref=r32,
                               factor=factor_of("readout"), report=report)
    finish(case, fails, report)
    nan_rows = d["layout"].startswith("dense") and d["mask"] is not None
    if not nan_rows:
        check_grads(case, kernel, lambda dt: FR.readout_reference(d, dt), ["x", "weight"])
    else:  # the same, with finite values on the masked rows (their gradient must be exact zeros)
        def kernel_finite():
            x = mv(d["x"]).requires_grad_(True)
            return _blocks(d, _readout_public(d, x)), {"x": x}
        check_grads(case, kernel_finite, lambda dt: FR.readout_reference(d, dt), ["x"])
        x = mv(d["x"]).requires_grad_(True)
        (gx,) = torch.autograd.grad(_readout_public(d, x).sum(), x)
        assert bool((gx[~mv(d["mask"])] == 0).all()), case


# ============================================================================================================== SAG
def _sag_x(d):
    if d["layout"] == "sliced":
        x = mv(d["x_base"])[:, d["first"]:d["first"] + d["F"]]
        assert x.stride(0) == d["F"] + 5
        return x
    return offset_by_one_element(mv(d["x"])) if d["layout"] == "offset" else mv(d["x"])


@pytest.mark.parametrize("seed", SEEDS)
def test_sag_operators(seed):
    from tgp import kernels as K
    d = FI.draw("sag", seed, limits())
    case, report = f"sag-op-{seed}", []
    x, ei, n = _sag_x(d), mv(d["edge_index"]), d["n"]
    w_rel, w_root, b = mv(d["w_rel"]), mv(d["w_root"]), mv(d["b"])
    p, q = K.row_project2(x, w_rel, w_rel if w_root is None else w_root)
    grp = K.sag_edge_group(ei, n, by_destination=True)
    ascending = bool((d["edge_index"][1, 1:] >= d["edge_index"][1, :-1]).all())
    assert ascending or d["order"] == "shuffled"
    assert (grp.perm is None) == ascending, case  # a list that ascends in its destinations needs only its CSR offsets
    t, a = K.sag_aggregate(grp, ei[0], p, None if w_root is None else q, b, mean=d["mean"], tanh=True, want_t=True)
    t2, a2 = K.sag_score(x, ei, w_rel, w_root, b, mean=d["mean"], tanh=True, want_t=True)
    assert torch.equal(t, t2) and torch.equal(a, a2), case
    assert torch.equal(K.sag_score(x, ei, w_rel, w_root, b, mean=d["mean"], tanh=False), t), case
    r64, r32 = FR.sag_reference(d, F64)[0], FR.sag_reference(d, F32)[0]
    with torch.no_grad():
        fails = forward_errors(case, {"p": p, "q": q, "t": t, "a": a}, r64, r32, factor=factor_of("sag"), report=report)
    # the native backward operator: dX = g_q (x) w_root + g_p (x) w_rel, alone and added to a gradient already there
    g_q, g_p = upstream(case + "q", n), upstream(case + "p", n)
    old = upstream(case + "old", n, d["F"]) if seed % 2 else None
    dx = K.sag_score_bwd_x(mv(g_q), mv(g_p), w_rel if w_root is None else w_root, w_rel,
                           None if old is None else mv(old).clone())

    def ref_dx(dtype):
        g = FR.sag_bwd_x_reference(d, dtype, g_q, g_p)
        return {"dx": g if old is None else g + old.to(dtype)}
    fails += forward_errors(case, {"dx": dx}, ref_dx(F64), ref_dx(F32), factor=factor_of("sag"), report=report)
    if seed % 4 == 0:
        again = K.sag_score(x, mv(d["edge_index"].clone()), w_rel, w_root, b, mean=d["mean"], tanh=True, want_t=True)
        assert torch.equal(t, again[0]) and torch.equal(a, again[1])
        by_src = K.sag_edge_group(ei, n, by_destination=False)
        gt = mv(g_q)
        assert torch.equal(K.sag_aggregate(by_src, ei[1], gt), K.sag_aggregate(by_src, ei[1], gt))
    finish(case, fails, report)


@pytest.mark.parametrize("seed", SEEDS)
def test_sag_public(seed):
    from tgp import functions as Fn
    d = FI.draw("sag", seed, limits())
    case, report = f"sag-public-{seed}", []
    ei = mv(d["edge_index"])

    def kernel():
        lv = {"x": _sag_x(d).detach().requires_grad_(True), "w_rel": mv(d["w_rel"]).requires_grad_(True),
              "w_root": None if d["w_root"] is None else mv(d["w_root"]).requires_grad_(True),
              "b": None if d["b"] is None else mv(d["b"]).requires_grad_(True)}
        a = Fn.sag_score(lv["x"], ei, lv["w_rel"], lv["w_root"], lv["b"], d["mean"], True)
        assert "_SagScoreFnBackward" in _graph_names(a.grad_fn)
        return {"a": a}, lv

    def oracle(dtype):
        outs, lv = FR.sag_reference(d, dtype)
        return {"a": outs["a"]}, lv
    outs, _ = kernel()
    with torch.no_grad():
        fails = forward_errors(case, outs, oracle(F64)[0], oracle(F32)[0], factor=factor_of("sag"), report=report)
    finish(case, fails, report)
    check_grads(case, kernel, oracle, ["x", "w_rel", "w_root", "b"])
    if seed % 4 == 0:
        runs = []
        for _ in range(2):
            o, lv = kernel()
            leaves = [t for t in lv.values() if t is not None]
            runs.append([o["a"].detach()] + list(torch.autograd.grad(o["a"].sum(), leaves)))
        assert all(torch.equal(u, v) for u, v in zip(*runs)), case


# ======================================================================================================== selectors
def _kmis_got(res, n):
    assert torch.equal(res.index[0], torch.arange(n, device=res.index.device))
    return {"k": torch.tensor(res.k), "mis": res.mis, "cluster": res.index[1]}


def _ec_got(res, n):
    assert torch.equal(res.index[0], torch.arange(n, device=res.index.device))
    return {"k": torch.tensor(res.k), "matched": res.matched, "match": res.match, "cluster": res.index[1]}


@pytest.mark.parametrize("seed", SEEDS)
def test_kmis_select(seed):
    from tgp import kernels as K
    d = FI.draw("kmis", seed, limits())
    case = f"kmis-{seed}"
    ei, n, k = mv(d["edge_index"]), d["n"], d["order_k"]
    ptr, gmax = mv(d["graph_ptr"]), d["max_graph_nodes"]
    assert K.kmis_route(n, ei.size(1), ptr, gmax) == d["route"], case
    fails = []
    for what, pri, perm in (("perm", dict(perm=mv(d["perm"])), d["perm"]),
                            ("score", dict(score=mv(d["score"]), heuristic=None), FR.tied_order(d["score"]))):
        want = FR.kmis_exact(d, perm)
        for route in (None, "rounds"):
            res = K.kmis_select(ei, n, k, graph_ptr=ptr, max_graph_nodes=gmax, route=route, **pri)
            assert res.route == (d["route"] if route is None else "rounds"), (case, what, route, res.route)
            fails += forward_errors(f"{case}-{what}-{route or 'natural'}", _kmis_got(res, n), want, want, exact=set(want))
            if seed % 4 == 0:
                two = K.kmis_select(ei, n, k, graph_ptr=ptr, max_graph_nodes=gmax, route=route, **pri)
                assert torch.equal(res.index, two.index) and torch.equal(res.mis, two.mis) and res.k == two.k
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("seed", SEEDS)
def test_edge_contract_select(seed):
    import edgepool_restatement as RE
    from tgp import kernels as K
    d = FI.draw("edge_contract", seed, limits())
    case = f"edge_contract-{seed}"
    ei, n = mv(d["edge_index"]), d["n"]
    ptr, gmax = mv(d["graph_ptr"]), d["max_graph_nodes"]
    assert K.edge_contract_route(n, ei.size(1), ptr, gmax) == d["route"], case
    fails = []
    for what, pri, perm in (("perm", dict(perm=mv(d["perm"])), d["perm"]),
                            ("score", dict(score=mv(d["score"])), FR.tied_order(d["score"]))):
        want = FR.edge_contract_exact(d, perm)
        if what == "score":  # the matched entry's score for both members of a pair, 1 for a singleton: copies
            want["weight"] = RE.weights(d["edge_index"], n, want["matched"].bool(), d["score"])
        for route in (None, "rounds"):
            res = K.edge_contract_select(ei, n, graph_ptr=ptr, max_graph_nodes=gmax, route=route, **pri)
            assert res.route == (d["route"] if route is None else "rounds"), (case, what, route, res.route)
            got = _ec_got(res, n)
            if what == "score":
                got["weight"] = res.weight
            fails += forward_errors(f"{case}-{what}-{route or 'natural'}", got, want, want, exact=set(want))
            m = want["matched"].bool()
            medge = res.medge.cpu()
            pairs = d["edge_index"][:, m]
            assert bool((medge[pairs[0]] == m.nonzero().view(-1)).all()) and bool((medge[pairs[1]] == m.nonzero().view(-1)).all())
            assert int((medge >= 0).sum()) == torch.unique(pairs).numel()
            if seed % 4 == 0:
                two = K.edge_contract_select(ei, n, graph_ptr=ptr, max_graph_nodes=gmax, route=route, **pri)
                assert torch.equal(res.index, two.index) and torch.equal(res.matched, two.matched) and res.k == two.k
    assert not fails, "\n".join(fails)


# ============================================================================================= the edge-group index
def _check_groups(case, ei_host, ei, n):
    """``kernels.sag_edge_group`` in both directions against a stable host argsort of the same list: the offsets, the
    positions (or their absence on a list that ascends in the grouped row) and the longest group, exactly."""
    from tgp import kernels as K
    fails, groups, E = [], {}, ei_host.size(1)
    for by_dst in (True, False):
        grp = K.sag_edge_group(ei, n, by_destination=by_dst)
        want = FR.edge_group_exact(ei_host, n, by_dst)
        where = f"{case}-{'by_dst' if by_dst else 'by_src'}"
        assert (grp.perm is None) == (want["perm"] is None), where
        assert grp.nnz == E and grp.num_targets == n and grp.max_members == want["max_members"], where
        ref = {"row_ptr": want["row_ptr"]}
        got = {"row_ptr": grp.row_ptr}
        if want["perm"] is not None:
            ref["perm"], got["perm"] = want["perm"], grp.perm[:E]
        fails += forward_errors(where, got, ref, ref, exact=set(ref))
        groups[by_dst] = grp
    return fails, groups[True], groups[False]


def _regrouped(d, by_dst):
    """The draw with its list in the other index form of that direction, every group's edges in the same order."""
    order = FR.regrouped_order(d["edge_index"], by_dst)
    v = dict(d)
    v["edge_index"] = d["edge_index"][:, order].contiguous()
    for name in ("edge_weight", "alpha_mask"):
        if d.get(name) is not None:
            v[name] = d[name][order].contiguous()
    return v, order


def _by_graph(d, outs, names):
    """``outs`` plus, for every listed per-node output, its rows graph by graph: no graph is judged through the batch."""
    res = dict(outs)
    for name in names:
        for b, c in enumerate(d.get("all_sizes", d["sizes"])):
            if c and name in outs:
                res[f"{name}[{b}]"] = outs[name][int(d["ptr"][b]):int(d["ptr"][b + 1])]
    return res


def _grads(y, leaves, up):
    """d<y, up> / d leaf for every leaf, zeros where the path does not reach it."""
    live = [t for t in leaves if t is not None]
    got = torch.autograd.grad(y, live, up.to(y.dtype), allow_unused=True, retain_graph=True) if y.requires_grad and live else ()
    got = iter(got)
    out = []
    for t in leaves:
        g = None if t is None else next(got, None)
        out.append(torch.zeros_like(t) if (g is None and t is not None) else g)
    return out


# ============================================================================================================= ASAP
def _rows_view(t, layout):
    """Host rows [n, F] as the device view of the drawn layout (tests/test_gpu_asap.py ``rows``): a column slice one
    float past a 16-byte boundary (row stride F + 3), a column slice that keeps the 16-byte loads (row stride the next
    multiple of four above F + 3), or contiguous but 4 bytes into its buffer.  The columns outside a slice hold NaN."""
    t = mv(t)
    n, f = t.shape
    if layout == "offset":
        return offset_by_one_element(t)
    if layout.startswith("sliced"):
        width, first = (f + 3, 1) if layout == "sliced_unaligned" else ((f + 7) // 4 * 4, 0)
        base = torch.full((n, width), float("nan"), device=t.device)
        base[:, first:first + f] = t
        view = base[:, first:first + f]
        assert view.stride(0) == width and view.data_ptr() % 16 == 4 * first
        return view
    return t


def _asap_form(x):
    """The load form the row kernels take for ``x``: the library's rule restated from F, the row stride and the pointer."""
    ld = x.stride(0) if x.size(0) > 1 else max(x.stride(0), x.size(1))
    return "vec16" if x.size(1) >= 4 and ld % 4 == 0 and x.data_ptr() % 16 == 0 else "scalar"


def _asap_operators(d, case, report, twice):
    from tgp import kernels as K
    fac = factor_of("asap")
    n, F, E, slope = d["n"], d["F"], d["edge_index"].size(1), d["negative_slope"]
    ei = mv(d["edge_index"])
    src, dst = ei[0], ei[1]
    fails, by_dst, by_src = _check_groups(case, d["edge_index"], ei, n)
    x = _rows_view(d["x"], d["layout"])
    x_pool = x if d["same_pool"] else _rows_view(d["x_pool"], d["layout"])
    assert _asap_form(x) == d["form"] and _asap_form(x_pool) == d["form"], (case, d["layout"], F)
    assert d["lanes"] == FI.asap_lanes(F, d["form"])
    inp = FR.asap_operator_inputs(d)
    wt, c, sq_in, sp_in, val, w3, p_in = (mv(inp[k]) for k in ("w_tilde", "c", "sq", "sp", "val", "w3", "p"))
    b1, b3, ew = mv(d["params"]["select_scorer.lin1.bias"]), mv(d["params"]["select_scorer.lin3.bias"]), mv(d["edge_weight"])

    def forward():
        sq, arg = K.asap_query(by_dst, src, x_pool, wt, c, want_arg=True)
        alpha = K.asap_edge_softmax(by_dst, src, sq_in, sp_in, slope)
        out, proj = K.asap_attend(by_dst, src, x, val, w3)
        t, a = K.asap_leconv(by_dst, src, p_in, ew, b1, b3, d["act"], want_t=True)
        return {"sq": sq, "alpha": alpha, "out": out, "proj": proj, "t": t, "a": a, "argpos": arg}
    got = forward()
    # without the table (the inference route folds the slots another way): the same bits
    same = {"sq without argpos": got["sq"]}
    fails += forward_errors(case, {"sq without argpos": K.asap_query(by_dst, src, x_pool, wt, c)}, same, same, exact=set(same))
    plain, none = K.asap_attend(by_dst, src, x, val)
    assert none is None and torch.equal(plain, got["out"]), case
    assert torch.equal(K.asap_leconv(by_dst, src, p_in, ew, b1, b3, d["act"]), got["a"]), case
    with torch.no_grad():
        r64, r32 = FR.asap_operator_reference(d, F64, inp)[0], FR.asap_operator_reference(d, F32, inp)[0]
    fails += forward_errors(case, got, r64, r32, factor=fac, report=report)
    # the arg-max table (the lowest position among equals, -1 for an empty group) and the maximum itself, exactly
    exact = FR.asap_argmax_exact(d)
    probe, zero = {"argpos": got["argpos"]}, torch.zeros(1, device=dev())
    cols = sorted({0, F // 2, F - 1})
    for f in cols:  # w~ = e_f, c = 0: sq is column f of the max row, an entry of the input
        e_f = torch.zeros(F, device=dev())
        e_f[f] = 1.0
        probe[f"max[:,{f}]"] = K.asap_query(by_dst, src, x_pool, e_f, zero)
        exact[f"max[:,{f}]"] = exact["max"][:, f]
    del exact["max"]
    fails += forward_errors(case, probe, exact, exact, exact=set(exact))
    if d["x_tied"] is not None:  # maxima held by several DIFFERENT source rows: forward only, the positions exactly
        tied = FR.asap_argmax_exact(d, d["x_tied"])
        _, arg = K.asap_query(by_dst, src, _rows_view(d["x_tied"], d["layout"]), wt, c, want_arg=True)
        fails += forward_errors(f"{case}-tied", {"argpos": arg}, {"argpos": tied["argpos"]}, tied, exact={"argpos"})
    # the four backward operators on seeded upstream gradients, against the float64 autograd of the same definitions
    g_out, g_alpha, g_sq = upstream(case + "g", n, F), upstream(case + "ga", E), upstream(case + "gsq", n)

    def backward():
        g_l, g_sq_out = K.asap_softmax_bwd(by_dst, src, got["alpha"], mv(g_alpha), sq_in, sp_in, slope)
        return {"g_x": K.asap_attend(by_src, dst, mv(g_out), val)[0], "g_val": K.asap_edge_dot(by_dst, src, mv(g_out), x),
                "g_l": g_l, "g_sq": g_sq_out, "g_x_pool": K.asap_query_bwd(by_src, dst, got["argpos"], mv(g_sq), wt)}

    def ref_backward(dtype):
        outs, lv = FR.asap_operator_reference(d, dtype, inp)
        g_x, g_val = _grads(outs["out"], [lv["x"], lv["val"]], g_out)
        g_l, g_sq_out = _grads(outs["alpha"], [lv["logit"], lv["sq_in"]], g_alpha)
        (g_xp,) = _grads(outs["sq"], [lv["x_pool"]], g_sq)
        return {"g_x": g_x, "g_val": torch.zeros(0, dtype=dtype) if g_val is None else g_val, "g_l": g_l,
                "g_sq": g_sq_out, "g_x_pool": g_xp}
    got_b = backward()
    fails += forward_errors(f"{case}-bwd", got_b, ref_backward(F64), ref_backward(F32), factor=fac, report=report)
    if twice:  # the same calls again: equal bits, forward and backward
        for first, second in ((got, forward()), (got_b, backward())):
            assert all(torch.equal(first[k], second[k]) for k in first), case
    return fails


@pytest.mark.parametrize("seed", SEEDS)
def test_asap_operators(seed):
    """Every ``tgp.kernels`` wrapper of csrc/asap.hip on the draw, one by one, each against its own plain definition:
    the index in both directions, the master query with its arg-max table, the edge softmax, the attend kernel with its
    projections, the LEConv aggregate, and the four backward operators."""
    d = FI.draw("asap", seed, limits())
    case, report = f"asap-op-{seed}", []
    fails = _asap_operators(d, case, report, seed % 4 == 0)
    if seed % 4 == 0:  # the same list in the other index form of its by-destination groups: within the bound as well
        fails += _asap_operators(_regrouped(d, True)[0], f"{case}-regrouped", report, False)
    finish(case, fails, report)


class _Calls:
    """Counts the calls of functions of a module while a block runs (which route a public class took)."""

    def __init__(self, owner, *names):
        self.owner, self.names, self.count = owner, names, {n: 0 for n in names}

    def __enter__(self):
        self._orig = {n: getattr(self.owner, n) for n in self.names}
        for n in self.names:
            def counted(*a, _n=n, **k):
                self.count[_n] += 1
                return self._orig[_n](*a, **k)
            setattr(self.owner, n, counted)
        return self

    def __exit__(self, *exc):
        for n, fn in self._orig.items():
            setattr(self.owner, n, fn)


@pytest.mark.parametrize("seed", SEEDS)
def test_asap_public(seed):
    """``functions.asap_attention`` + ``asap_leconv_score`` (one autograd node each) against the REFERENCE-SHAPED
    restatement: values graph by graph, gradients one output at a time to x, x_pool and every drawn parameter; the same
    through ``ASAPooling.fitness`` and the whole pooler where the draw is one the class takes (every bias on, x_pool = x;
    the pooler: no mask), what follows the selection on the product's own kept nodes."""
    import asap_restatement as RAS
    from tgp import functions as Fn
    from tgp.poolers import ASAPooling
    d = FI.draw("asap", seed, limits())
    case, report, fac = f"asap-public-{seed}", [], factor_of("asap")
    ei, ew, mask, slope = mv(d["edge_index"]), mv(d["edge_weight"]), mv(d["alpha_mask"]), d["negative_slope"]
    names = [k for k, v in d["params"].items() if v is not None]

    def leaves(view):
        x = _rows_view(d["x"], view["layout"]).detach().requires_grad_(True)
        x_pool = x if d["same_pool"] else _rows_view(d["x_pool"], view["layout"]).detach().requires_grad_(True)
        return x, x_pool, {k: mv(d["params"][k]).requires_grad_(True) for k in names}

    def run(x, x_pool, par, edges, weight, msk):
        w3 = torch.cat([par[f"select_scorer.lin{k}.weight"] for k in (1, 2, 3)])
        alpha, x_new, p = Fn.asap_attention(x, x_pool, edges, par["lin.weight"], par.get("lin.bias"), par["att.weight"],
                                            par.get("att.bias"), slope, msk, w3)
        score = Fn.asap_leconv_score(x_new, edges, weight, w3, par.get("select_scorer.lin1.bias"),
                                     par.get("select_scorer.lin3.bias"), d["act"], p)
        return {"alpha": alpha, "x_new": x_new, "score": score}

    def kernel():
        x, x_pool, par = leaves(d)
        outs = run(x, x_pool, par, ei, ew, mask)
        assert "_AsapAttentionFnBackward" in _graph_names(outs["x_new"].grad_fn), case
        assert "_AsapLeconvFnBackward" in _graph_names(outs["score"].grad_fn) and not outs["alpha"].requires_grad, case
        return outs, {"x": x, "x_pool": x_pool, **par}

    def oracle(dtype):
        return FR.asap_reference(d, dtype)
    assert _asap_form(leaves(d)[0]) == d["form"], case
    outs, _ = kernel()
    rows = ("x_new", "score")
    with torch.no_grad():
        r64, r32 = _by_graph(d, oracle(F64)[0], rows), _by_graph(d, oracle(F32)[0], rows)
        fails = forward_errors(case, _by_graph(d, outs, rows), r64, r32, factor=fac, report=report)
        x, x_pool, par = leaves(d)  # without a graph: the inference route (no arg-max table), held to the same bound
        plain = run(x.detach(), x_pool.detach(), {k: v.detach() for k, v in par.items()}, ei, ew, mask)
        fails += forward_errors(f"{case}-no-grad", _by_graph(d, plain, rows), r64, r32, factor=fac, report=report)
    finish(case, fails, report)
    lv_names = ["x", "x_pool"] + names
    check_grads(case, kernel, oracle, lv_names)
    if seed % 4 == 0:
        runs = []
        for _ in range(2):  # the same public call twice: equal bits, forward and backward
            o, lv = kernel()
            wrt = [lv["x"]] + ([] if d["same_pool"] else [lv["x_pool"]]) + [lv[k] for k in names]
            total = (o["x_new"] * o["score"].view(-1, 1)).sum()
            runs.append([o["alpha"], o["x_new"].detach(), o["score"].detach()] + list(torch.autograd.grad(total, wrt)))
        assert all(torch.equal(u, v) for u, v in zip(*runs)), case
        v, order = _regrouped(d, True)  # the other index form of the same list: within the bound as well
        x, x_pool, par = leaves(v)
        with torch.no_grad():
            other = run(x.detach(), x_pool.detach(), {k: t.detach() for k, t in par.items()}, mv(v["edge_index"]),
                        mv(v["edge_weight"]), mv(v["alpha_mask"]))
            want64, want32 = dict(r64, alpha=r64["alpha"][order]), dict(r32, alpha=r32["alpha"][order])
            more = []
            fails = forward_errors(f"{case}-regrouped", _by_graph(d, other, rows), want64, want32, factor=fac, report=more)
        finish(case, fails, more)
    if not (d["bias"] and d["same_pool"]):
        return
    # the public class on the draws it takes natively
    pool = ASAPooling(d["F"], ratio=0.5, negative_slope=slope, nonlinearity=d["act"]).to(dev()).eval()
    pool.load_state_dict({k: mv(t) for k, t in d["params"].items()})
    par = dict(pool.named_parameters())
    with _Calls(Fn, "asap_attention", "asap_leconv_score") as calls:
        x = _rows_view(d["x"], d["layout"]).detach().requires_grad_(True)
        alpha, x_new, score = pool.fitness(x, ei, ew, mask=mask, act=d["act"])
    assert calls.count == {"asap_attention": 1, "asap_leconv_score": 1}, (case, calls.count)  # the native route
    assert "_AsapAttentionFnBackward" in _graph_names(x_new.grad_fn) and "_AsapLeconvFnBackward" in _graph_names(score.grad_fn)
    for name, t in (("alpha", alpha), ("x_new", x_new), ("score", score)):
        assert torch.equal(t.detach(), outs[name].detach()), (case, name)  # the functions' own bits
    if d["alpha_mask"] is not None:
        return
    # the whole pooler: Reduce on the PRODUCT's kept nodes (TopK's choice among float scores is not compared)
    batch, kept = mv(d["batch"]), {}

    def pooler():
        x = _rows_view(d["x"], d["layout"]).detach().requires_grad_(True)
        with _Calls(Fn, "asap_attention") as calls:
            out = pool(x=x, adj=ei, edge_weight=ew, batch=batch)
        assert calls.count["asap_attention"] == 1, case
        perm = torch.empty_like(out.so.node_index)
        perm[out.so.cluster_index] = out.so.node_index  # row c of the pooled features is the kept node of supernode c
        kept["perm"] = perm.cpu()
        return {"x_pool": out.x}, {"x": x, **par}
    pooler()
    fixture = FR.asap_pool_case(d)

    def pooled(dtype):
        x = d["x"].to(dtype).requires_grad_(True)
        p = {k: t.to(dtype).requires_grad_(True) for k, t in d["params"].items()}
        got = RAS.pool_case(fixture, dtype, collapsed=False, params=p, x=x, perm=kept["perm"])
        return {"x_pool": got["x_pool"]}, {"x": x, **p}
    more = []
    with torch.no_grad():
        fails = forward_errors(f"{case}-pooler", pooler()[0], pooled(F64)[0], pooled(F32)[0], factor=fac, report=more)
    finish(case, fails, more)
    # (where no kept node's group holds logits on both sides of 0, the pooled rows do not depend on the query half of
    # the attention in exact arithmetic: its parameters are then no leaves of this path)
    query_half = () if FR.asap_query_half_matters(d, kept["perm"]) else ("lin.weight", "lin.bias", "att.bias")
    check_grads(f"{case}-pooler", pooler, pooled, ["x"] + [k for k in names if k not in query_half])


# =========================================================================================================== MaxCut
def _maxcut_lists(d):
    """The score net's parameters of the draw as ``functions.maxcut_score`` takes them, by the reference's names."""
    import maxcut_restatement as RM
    pre, depth, n_mlp = RM.PRE, len(d["widths"]), len(d["mlp_units"])
    tail = [f"{pre}mlp.{l}{e}" for l in range(n_mlp) for e in (".weight", ".bias")] \
        + [pre + "final_layer.weight", pre + "final_layer.bias"]
    return ([pre + "initial_layer.weight", pre + "initial_layer.bias"], [f"{pre}mp_convs.{l}.lin.weight" for l in range(depth)],
            [f"{pre}mp_convs.{l}.bias" for l in range(depth)], tail)


def _maxcut_operators(d, case, report, twice, inp=None, seeds=None):
    """(failures, every output by name, the operators' float32 inputs) of the ``tgp.kernels`` wrappers of
    csrc/maxcut.hip on the draw, one by one.  ``inp``: the inputs of another run (the same list in another order: the
    host's own dinv would be summed in that other order); ``seeds``: that run's case, which names its upstream gradients."""
    import types

    import maxcut_restatement as RM
    from tgp import kernels as K
    fac = factor_of("maxcut")
    n, E, delta, widths = d["n"], d["edge_index"].size(1), d["delta"], d["widths"]
    ei = mv(d["edge_index"])
    row, col = ei[0], ei[1]
    fails, by_dst, by_src = _check_groups(case, d["edge_index"], ei, n)
    ew, par = mv(d["edge_weight"]), {k: mv(v) for k, v in d["params"].items()}
    inp = FR.maxcut_operator_inputs(d) if inp is None else inp
    w32 = RM._weights(d["edge_index"], d["edge_weight"], F32)
    dinv_in = mv(inp["dinv"])
    coef_in, coef_t_in = mv(w32 * inp["dinv"][d["edge_index"][0]]), mv(w32 * inp["dinv"][d["edge_index"][1]])
    n_p = K.maxcut_n_p(ei)
    assert int(n_p) == d["n_p"], case
    place = offset_by_one_element if d["layout"] == "offset" else (lambda t: t)
    g_t = [upstream(f"{seeds or case}gt{l}", n, c) for l, c in enumerate(widths)]
    _, conv_w, conv_b, tail = _maxcut_lists(d)
    s = mv(d["s"])

    def forward():
        dinv, coef, coef_t = K.maxcut_degree(by_src, ei, ew, True, True)
        got = {"dinv": dinv, "coef": coef, "coef_t": coef_t}
        for l in range(len(widths)):
            z = place(mv(inp["z"][l]))
            w_next = par[conv_w[l + 1]] if l + 1 < len(widths) else None
            h, zn = K.maxcut_layer(by_dst, row, coef_in, dinv_in, z, par[conv_b[l]], n_p, delta, d["mp_act"], w_next)
            got[f"h{l}"] = h
            if w_next is not None:
                got[f"z_next{l}"] = zn
                none, again = K.maxcut_layer(by_dst, row, coef_in, dinv_in, z, par[conv_b[l]], n_p, delta, d["mp_act"],
                                             w_next, want_h=False)
                assert none is None and torch.equal(again, zn), (case, l)  # without h: the same bits
            got[f"lin{l}"] = K.maxcut_layer(by_dst, row, coef_in, dinv_in, z, None, n_p, delta, "identity")[0]
            # the backward's use: the by-source group with w_e dinv[dst_e], no bias, no activation, g_h_prev = g_z W fused
            back = par[conv_w[l]].t().contiguous() if l > 0 else None
            got[f"g_z{l}"], g_h = K.maxcut_layer(by_src, col, coef_t_in, dinv_in, place(mv(g_t[l])), None, n_p, delta,
                                                 "identity", back, want_h=True)
            if l > 0:
                got[f"g_h{l}"] = g_h
        if d["tail"] != "unfit":
            got["tail"] = K.maxcut_tail(mv(inp["h_tail"]), [par[k] for k in tail[0::2]], [par[k] for k in tail[1::2]],
                                        d["mlp_act"], d["act"])
        got["az"], got["cut"], got["wsum"] = K.maxcut_cut(by_src, col, s, ew)
        at = K.maxcut_cut(by_dst, row, s, ew, want_cut=False, want_wsum=False)
        assert at[1] is None and at[2] is None
        got["at"] = at[0]
        labels = torch.zeros(n, dtype=torch.int32, device=dev())
        labels[mv(d["kept"])] = torch.arange(1, d["kept"].numel() + 1, dtype=torch.int32, device=dev())
        got["labels"] = K.maxcut_assign_rounds(by_dst, row, labels, d["max_iter"])
        return got

    def reference(dtype):
        outs, lv = FR.maxcut_operator_reference(d, dtype, inp)
        for l in range(len(widths)):
            (outs[f"g_z{l}"],) = _grads(outs[f"lin{l}"], [lv[f"z{l}"]], g_t[l])
            if l > 0:
                outs[f"g_h{l}"] = outs[f"g_z{l}"] @ d["params"][conv_w[l]].to(dtype)
        return {k: v.detach() for k, v in outs.items()}
    got = forward()
    layers = [types.SimpleNamespace(weight=d["params"][w], bias=d["params"][b]) for w, b in zip(tail[0::2], tail[1::2])]
    assert K.maxcut_tail_fits(widths[-1], layers) == (d["tail"] != "unfit"), case
    if d["zero_degree_node"] is not None:  # its degree is 0 although it has edges: inf -> 0
        assert float(got["dinv"][d["zero_degree_node"]]) == 0.0, case
    r64, r32 = reference(F64), reference(F32)
    exact = {"labels": FR.maxcut_labels_exact(d)}
    fails += forward_errors(case, got, {**r64, **exact}, r32, exact={"labels"}, factor=fac, report=report)
    # the weight gradient a^T b at the drawn N and around the rows of one partial sum
    ca, cb = widths[-1], d["F"]
    for rows in [n] + (d["wgrad_rows"] if not case.endswith("regrouped") else []):
        a, b = upstream(f"{case}wa{rows}", rows, ca), upstream(f"{case}wb{rows}", rows, cb)
        name = "wgrad" if rows == n else f"wgrad@{rows}"
        got[name] = K.maxcut_wgrad(mv(a), mv(b))
        fails += forward_errors(case, {name: got[name]}, {name: a.double().t() @ b.double()}, {name: a.t() @ b}, factor=fac,
                                report=report)
        if twice:
            assert torch.equal(got[name], K.maxcut_wgrad(mv(a), mv(b))), (case, name)
    if twice:
        again = forward()
        assert all(torch.equal(got[k], again[k]) for k in again), case
    return fails, got, inp


@pytest.mark.parametrize("seed", SEEDS)
def test_maxcut_operators(seed):
    """Every ``tgp.kernels`` wrapper of csrc/maxcut.hip on the draw: the index in both directions, the degrees with both
    coefficient arrays, every drawn layer (h, the fused projection to the next layer's width, the form without h, the
    backward's use over the by-source group), the tail, the weight gradient, the cut kernel in both directions and the
    assignment rounds (exactly).  One seed in four: the same calls twice, and the list in the other index form of its
    by-destination and of its by-source groups -- EQUAL bits in everything that is summed over those groups."""
    d = FI.draw("maxcut", seed, limits())
    case, report = f"maxcut-op-{seed}", []
    fails, got, inp = _maxcut_operators(d, case, report, seed % 4 == 0)
    if seed % 4 == 0:
        depth = len(d["widths"])
        sums = {True: [f"{n}{l}" for l in range(depth) for n in ("h", "lin")] + [f"z_next{l}" for l in range(depth - 1)]
                + ["at", "labels"],
                False: ["dinv", "az", "cut", "wsum"] + [f"g_z{l}" for l in range(depth)] + [f"g_h{l}" for l in range(1, depth)]}
        for by_dst in (True, False):
            v, order = _regrouped(d, by_dst)
            more, other, _ = _maxcut_operators(v, f"{case}-{'dst' if by_dst else 'src'}-regrouped", report, False, inp, case)
            fails += more
            for name in sums[by_dst]:
                assert torch.equal(got[name], other[name]), (case, by_dst, name)
            if not by_dst:
                for name in ("coef", "coef_t"):
                    assert torch.equal(got[name][mv(order)], other[name]), (case, name)
    finish(case, fails, report)


@pytest.mark.parametrize("seed", SEEDS)
def test_maxcut_public(seed):
    """``functions.maxcut_score`` and ``functions.maxcut_loss`` (one autograd node each) against the REFERENCE-SHAPED
    score net (the explicit delta-GCN matrix) and ``cut_loss``: values (the scores graph by graph), gradients one output
    at a time to x, s and every parameter; the same through ``MaxCutScoreNet`` and ``utils.maxcut_loss`` with their
    routes -- a tail that does not fit the kernels takes the composed form --, and ``MaxCutSelect.assign`` on the drawn
    kept nodes (the labelled nodes only: the draw for the others is not compared)."""
    import maxcut_restatement as RM
    from tgp import functions as Fn
    from tgp import kernels as K
    from tgp.poolers import MaxCutScoreNet, MaxCutSelect
    from tgp.select import SelectOutput
    from tgp.utils import maxcut_loss
    d = FI.draw("maxcut", seed, limits())
    case, report, fac = f"maxcut-public-{seed}", [], factor_of("maxcut")
    fits, n, sizes = d["tail"] != "unfit", d["n"], d["all_sizes"]
    ei, ew, batch = mv(d["edge_index"]), mv(d["edge_weight"]), mv(d["batch"])
    names = sorted(d["params"])
    init, conv_w, conv_b, tail = _maxcut_lists(d)
    nb = int(d["batch"].max()) + 1  # (the graphs the batch vector shows: an empty graph at the end is not among them)
    ptr, longest = mv(d["ptr"][:nb + 1]), max(sizes[:nb])
    place = offset_by_one_element if d["layout"] == "offset" else (lambda t: t)

    def leaves():
        return place(mv(d["x"])).requires_grad_(True), mv(d["s"]).requires_grad_(True), \
            {k: mv(d["params"][k]).requires_grad_(True) for k in names}

    def score_of(x, par, edges, weight):
        return Fn.maxcut_score(x, edges, weight, [par[k] for k in init], [par[k] for k in conv_w], [par[k] for k in conv_b],
                               [par[k] for k in tail], d["delta"], d["mp_act"], d["mlp_act"], d["act"])

    net = MaxCutScoreNet(d["F"], mp_units=d["widths"], mp_act=d["mp_act"], mlp_units=d["mlp_units"], mlp_act=d["mlp_act"],
                         act=d["act"], delta=d["delta"]).to(dev())
    net.load_state_dict({k[len(RM.PRE):]: mv(v) for k, v in d["params"].items()})
    net_par = {RM.PRE + k: v for k, v in net.named_parameters()}
    assert sorted(net_par) == names

    def kernel():
        x, s, par = leaves()
        if fits:
            score = score_of(x, par, ei, ew)
            assert "_MaxCutScoreFnBackward" in _graph_names(score.grad_fn), case
        else:  # the class is the only public form of a net the kernels do not take: the composed route
            with _Calls(Fn, "maxcut_score") as calls:
                score = net(x, ei, ew).view(-1)
            assert calls.count["maxcut_score"] == 0 and "_MaxCutScoreFnBackward" not in _graph_names(score.grad_fn), case
            par = net_par
        loss = Fn.maxcut_loss(s, ei, ew, batch, ptr, nb, longest)
        assert "_MaxCutLossFnBackward" in _graph_names(loss.grad_fn), case
        return {"score": score, "loss": loss}, {"x": x, "s": s, **par}

    def oracle(dtype):
        return FR.maxcut_reference(d, dtype)
    assert net.native_case(place(mv(d["x"])), ei, ew) == fits, case
    outs, _ = kernel()
    with torch.no_grad():
        r64, r32 = _by_graph(d, oracle(F64)[0], ("score",)), _by_graph(d, oracle(F32)[0], ("score",))
        fails = forward_errors(case, _by_graph(d, outs, ("score",)), r64, r32, factor=fac, report=report)
        # without a graph: the inference route (only the last layer's h is written, the tail kernel scores the rows)
        with _Calls(Fn, "maxcut_score", "maxcut_loss") as calls:
            plain = {"score": net(place(mv(d["x"])), ei, ew).view(-1), "loss": maxcut_loss(mv(d["s"]), ei, ew, batch)}
        assert calls.count == {"maxcut_score": int(fits), "maxcut_loss": 1}, (case, calls.count)
        assert torch.equal(plain["loss"], outs["loss"].detach()), case
        fails += forward_errors(f"{case}-no-grad", _by_graph(d, plain, ("score",)), r64, r32, factor=fac, report=report)
    finish(case, fails, report)
    check_grads(case, kernel, oracle, ["x", "s"] + names)
    if fits:  # the class under autograd: the functions' node and its bits
        x, _, _ = leaves()
        with _Calls(Fn, "maxcut_score") as calls:
            tracked = net(x, ei, ew).view(-1)
        assert calls.count["maxcut_score"] == 1 and "_MaxCutScoreFnBackward" in _graph_names(tracked.grad_fn), case
        assert torch.equal(tracked.detach(), outs["score"].detach()), case
    if seed % 4 == 0 and fits:
        runs = []
        for _ in range(2):  # the same public call twice: equal bits, forward and backward
            o, lv = kernel()
            wrt = [lv["x"], lv["s"]] + [lv[k] for k in names]
            runs.append([o["score"].detach(), o["loss"].detach()] + list(torch.autograd.grad(o["score"].sum() + o["loss"], wrt)))
        assert all(torch.equal(u, v) for u, v in zip(*runs)), case
        v, _ = _regrouped(d, True)  # the other index form of the by-destination groups: within the bound as well
        with torch.no_grad():
            x, s, par = leaves()
            e2, w2 = mv(v["edge_index"]), mv(v["edge_weight"])
            other = {"score": score_of(x.detach(), {k: t.detach() for k, t in par.items()}, e2, w2),
                     "loss": Fn.maxcut_loss(s.detach(), e2, w2, batch, ptr, nb, longest)}
            more = []
            fails = forward_errors(f"{case}-regrouped", _by_graph(d, other, ("score",)), r64, r32, factor=fac, report=more)
        finish(case, fails, more)
    # the assignment through the selector: native rounds unless every node is kept; the labelled nodes exactly
    kept = mv(d["kept"])
    sel = MaxCutSelect(4, mp_units=[4], mlp_units=[])
    so = SelectOutput(node_index=kept, num_nodes=n, cluster_index=torch.arange(kept.numel(), device=dev()),
                      num_supernodes=kept.numel())
    with _Calls(K, "maxcut_assign_rounds") as calls:
        got = sel.assign(so, ei, None, batch, d["max_iter"])
    assert calls.count["maxcut_assign_rounds"] == int(kept.numel() < n), (case, calls.count)
    label = FR.maxcut_labels_exact(d)
    reached = label > 0
    assert got.num_supernodes == kept.numel() and got.num_nodes == n, case
    assert torch.equal(got.cluster_index.cpu()[reached], label[reached] - 1), case
    if d["chain"]:
        assert int((~reached).sum()) > 0, case  # the path's tail is left to the draw inside its graph


# ========================================================================================================== GTVConv
GTV_ROWS = ("out", "g", "dh")  # the per-node outputs, also judged graph by graph


def _gtv_form(h, C):
    """The load form the register kernels take for rows ``h`` (fresh outputs are 16-byte aligned)."""
    return "vec16" if C % 4 == 0 and h.data_ptr() % 16 == 0 else "scalar"


def _gtv_took_native(before, case):
    from tgp import kernels as K
    after = K.gtv_record()
    assert after["route"] == "native" and after["native"] == before["native"] + 1 \
        and after["composed"] == before["composed"], (case, before, after)


def _gtv_operators(d, case, report, twice):
    from tgp import kernels as K
    fac = factor_of("gtv")
    n, C, E = d["n"], d["C"], d["edge_index"].size(1)
    ei = mv(d["edge_index"])
    row, col = K._edge_rows(ei)
    fails, by_dst, by_src = _check_groups(case, d["edge_index"], ei, n)
    h = offset_by_one_element(mv(d["h"])) if d["layout"] == "offset" else mv(d["h"])
    assert _gtv_form(h, C) == d["form"] and h.is_contiguous(), (case, d["layout"], C)
    w, bias, mask = mv(d["edge_weight"]), mv(d["bias"]), mv(d["mask"])
    code, delta, eps = K.GTV_ACT_CODES[d["act"]], d["delta"], d["eps"]
    g_out = mv(FR.upstream(case + "g", n, C))

    def run():
        out, dist = K.gtv_edge_fwd(h, col, w, by_src, bias, mask, delta, eps, code, want_d=True)
        g, gw, t = K.gtv_edge_bwd_terms(h, out, g_out, col, w, by_src, dist, mask, delta, eps, code, want_gw=True)
        dh = K.gtv_edge_bwd_nodes(h, g, row, col, w, by_src, by_dst, dist, t, delta, eps)
        return {"out": out, "d": dist, "g": g, "gw": gw, "dh": dh, "t": t}
    got = run()
    plain, none = K.gtv_edge_fwd(h, col, w, by_src, bias, mask, delta, eps, code)  # without the distances: the same bits
    assert none is None and torch.equal(plain, got["out"]), case
    r64, r32 = (_by_graph(d, FR.gtv_operator_reference(d, dt, case)[0], GTV_ROWS) for dt in (F64, F32))
    skipped = FR.gtv_skipped(d)
    zeros = {"d": skipped, "gw": skipped}
    if d["mask"] is not None:  # every row of a masked node: exact zeros in out and g
        zeros["out"] = zeros["g"] = (~d["mask"]).view(-1, 1).expand(n, C)
    # t, the gradient at the distances, has no output in the restatement: the terms kernel's own formula written out
    # (``gtv_backward_by_hand``, which tests/test_fuzz_inputs.py holds to autograd through dh) isolates it from the node kernel
    for ref, dt in ((r64, F64), (r32, F32)):
        ref["t"] = FR.gtv_backward_by_hand(d, dt, case)["t"]
    zeros["t"] = skipped
    fails += forward_errors(case, _by_graph(d, got, GTV_ROWS), r64, r32, zeros=zeros, factor=fac, report=report)
    if twice:
        again = run()
        assert all(torch.equal(v, again[k]) for k, v in got.items()), case
    return fails


@pytest.mark.parametrize("seed", SEEDS)
def test_gtv_operators(seed):
    """``gtv_edge_fwd(want_d=True)``, then ``gtv_edge_bwd_terms(want_gw=True)`` on the kernel's own ``out`` and ``d``, then
    ``gtv_edge_bwd_nodes`` on the terms kernel's ``g`` and ``t``, on both edge indexes as ``sag_edge_group`` builds them
    (compared exactly with a stable host argsort): out and d by the rule, g, gw and dh against float64 autograd's
    gradients at the activation input, the edge weights and h; exact zeros at skipped edges (d, gw, t) and in every row
    of a masked node (out, g)."""
    d = FI.draw("gtv", seed, limits())
    case, report = f"gtv-op-{seed}", []
    finish(case, _gtv_operators(d, case, report, seed % 4 == 0), report)


@pytest.mark.parametrize("seed", SEEDS)
def test_gtv_public(seed):
    """``GTVConv`` in sparse mode on the native route: values graph by graph, gradients to x, weight, bias and
    edge_weight; on two seeds the dense-mode call of the same batch (duplicates added up, loops on the diagonal, the
    padded rows masked) as well."""
    from tgp import kernels as K
    from tgp.mp import GTVConv
    d = FI.draw("gtv", seed, limits())
    case, report, fac = f"gtv-public-{seed}", [], factor_of("gtv")
    ei = mv(d["edge_index"])
    conv = GTVConv(FI.GTV_F_IN, d["C"], bias=d["bias"] is not None, delta_coeff=d["delta"], eps=d["eps"], act=d["act"]).to(dev())
    with torch.no_grad():
        conv.weight.copy_(mv(d["weight"]))
        if d["bias"] is not None:
            conv.bias.copy_(mv(d["bias"]))
    place = offset_by_one_element if d["layout"] == "offset" else (lambda t: t)

    def kernel():
        x = place(mv(d["x"])).requires_grad_(True)
        ew = None if d["edge_weight"] is None else mv(d["edge_weight"]).requires_grad_(True)
        before = K.gtv_record()
        out = conv(x, ei, ew)
        _gtv_took_native(before, case)
        assert "_GtvPropagateFnBackward" in _graph_names(out.grad_fn), case
        return {"out": out}, {"x": x, "weight": conv.weight, "bias": conv.bias, "edge_weight": ew}

    def oracle(dtype):
        return FR.gtv_reference(d, dtype)
    leaves = ["x", "weight"] + (["bias"] if d["bias"] is not None else []) + (["edge_weight"] if d["weighted"] else [])
    with torch.no_grad():
        before = K.gtv_record()
        out = conv(place(mv(d["x"])), ei, mv(d["edge_weight"]))
        _gtv_took_native(before, case)
        r64, r32 = _by_graph(d, oracle(F64)[0], ("out",)), _by_graph(d, oracle(F32)[0], ("out",))
    fails = forward_errors(case, _by_graph(d, {"out": out}, ("out",)), r64, r32, factor=fac, report=report)
    assert torch.equal(kernel()[0]["out"].detach(), out), case  # with and without the distance buffer: the same bits
    finish(case, fails, report)
    check_grads(case, kernel, oracle, leaves)
    if seed % 4 == 0:
        runs = []
        for _ in range(2):  # the same public call twice: equal bits, forward and backward
            o, lv = kernel()
            runs.append([o["out"].detach()] + list(torch.autograd.grad(o["out"], [lv[k] for k in leaves],
                                                                       mv(upstream(case, *o["out"].shape)))))
        assert all(torch.equal(u, v) for u, v in zip(*runs)), case
    if d["dense"]:
        dcase, more = f"{case}-dense", []
        x_p, adj, mask = (mv(t) for t in FR.gtv_dense_batch(d))

        def dense_kernel():
            x = x_p.clone().requires_grad_(True)
            before = K.gtv_record()
            out = conv(x, adj, mask=mask)
            _gtv_took_native(before, dcase)
            return {"out": out}, {"x": x, "weight": conv.weight, "bias": conv.bias}
        with torch.no_grad():
            got = {f"out[{b}]": t for b, t in enumerate(dense_kernel()[0]["out"])}
            want = [{f"out[{b}]": t for b, t in enumerate(FR.gtv_dense_reference(d, dt)[0]["out"])} for dt in (F64, F32)]
            pad = {f"out[{b}]": (~mask[b]).cpu().view(-1, 1).expand(mask.size(1), d["C"]) for b in range(d["B"])}
        finish(dcase, forward_errors(dcase, got, want[0], want[1], zeros=pad, factor=fac, report=more), more)
        check_grads(dcase, dense_kernel, lambda dt: FR.gtv_dense_reference(d, dt), leaves[:2 + (d["bias"] is not None)])


# ============================================================================================================== PAN
def _pan_split(d, ex, outs, kept=None):
    """``outs`` plus, graph by graph: M's values and ``part`` by the graph of the entry's row, per-node rows by the node's
    graph, the outputs on the kept nodes by the kept node's graph.  No graph is judged through the batch."""
    res, batch = dict(outs), d["batch"]
    groups = {"values": batch[ex["index"][0]], "met_values": batch[ex["index"][0]], "part": batch, "conv_out": batch}
    if kept is not None:
        groups.update(weight=batch[kept], x_pool=batch[kept])
    for name, owner in groups.items():
        if name in outs:
            for b in owner.unique().tolist():
                res[f"{name}[{b}]"] = outs[name][mv(owner == b) if outs[name].is_cuda else owner == b]
    return res


def _pan_score_x(d):
    """The scorer's x on the device: contiguous, or a column slice of a wider buffer (ldx = F + 3, NaN around it)."""
    x = mv(d["score_x"])
    if d["layout"] == "plain":
        return x
    base = torch.full((x.size(0), x.size(1) + 3), float("nan"), device=dev())
    base[:, 1:1 + x.size(1)] = x
    view = base[:, 1:1 + x.size(1)]
    assert view.stride(0) > x.size(1)
    return view


@pytest.mark.parametrize("seed", SEEDS)
def test_pan_operators(seed):
    """``pan_met`` (index and row_ptr exactly, values per graph), ``pan_met_bwd`` on a seeded upstream gradient (``part``
    per row against the float64 row-power form on the stored pattern, its column sums against autograd's gradient at the
    series coefficients) and ``pan_score(want_terms=True)`` on its own drawn inputs.  One node past the limit the MET
    matrix comes from the composed form (no frame, so no native backward) and still meets the rule."""
    from tgp import kernels as K
    from tgp.nn import PANConv
    d = FI.draw("pan", seed, limits())
    case, report, fac = f"pan-op-{seed}", [], factor_of("pan")
    n, L, sizes = d["n"], d["filter_size"], d["all_sizes"]
    ei, w = mv(d["edge_index"]), mv(d["weight"])
    gptr, gid = mv(d["ptr"]).to(torch.int32), mv(d["batch"]).to(torch.int32)
    native = d["route"] == "native"
    assert (K.pan_route(ei, w, n, gptr, max(sizes)) == "native") == native, case

    def met_of():
        if native:
            return K.pan_met(ei, w, n, gid, gptr, max(sizes))
        conv = PANConv(FI.PAN_F, FI.PAN_F, L).to(dev())
        with torch.no_grad():
            conv.weight.copy_(w)
            return conv.met(ei, n, mv(d["batch"]))
    met = met_of()
    assert met is not None and (met.frame is not None) == native, case
    ex = FR.pan_exact(d)
    r64, r32 = (FR.pan_operator_reference(d, dt, case)[0] for dt in (F64, F32))
    got = {"index": met.index, "row_ptr": met.row_ptr, "values": met.values}
    g = mv(FR.upstream(case + "g", ex["index"].size(1)))
    if native:
        got["part"] = K.pan_met_bwd(met, g)
        got["dc"] = got["part"].double().sum(0)
    else:
        r64, r32 = ({k: v for k, v in r.items() if k not in ("part", "dc")} for r in (r64, r32))
    col_group = K.edge_group(mv(d["score_index"]), n, by_destination=True)
    x, p, beta, vals = _pan_score_x(d), mv(d["score_p"]), mv(d["beta"]), mv(d["score_values"])
    got["score"], got["dot"], got["colsum"] = K.pan_score(x, p, beta, col_group, vals, d["use_tanh"], want_terms=True)
    assert torch.equal(K.pan_score(x, p, beta, col_group, vals, d["use_tanh"]), got["score"]), case
    want = dict(_pan_split(d, ex, r64), index=ex["index"], row_ptr=ex["row_ptr"])
    fails = forward_errors(case, _pan_split(d, ex, got), want, _pan_split(d, ex, r32), exact={"index", "row_ptr"},
                           factor=fac, report=report)
    if seed % 4 == 0:
        again = met_of()
        assert torch.equal(again.index, met.index) and torch.equal(again.values, met.values), case
        assert not native or torch.equal(K.pan_met_bwd(again, g), got["part"]), case
        terms = K.pan_score(x, p, beta, col_group, vals, d["use_tanh"], want_terms=True)
        assert all(torch.equal(t, got[k]) for t, k in zip(terms, ("score", "dot", "colsum"))), case
    finish(case, fails, report)


@pytest.mark.parametrize("seed", SEEDS)
def test_pan_public(seed):
    """``PANConv`` -> ``PANPooling``: conv_out and M's values graph by graph, the kept set, M's index and the pooled
    matrix's index exactly, the kept nodes' weights, x_pool and the pooled values (in ascending node order: the order
    among the kept is not compared, the draw keeps only the cut clear of rounding), and the gradients one output at a
    time to x, the series weights, ``lin``, ``p`` and ``beta``."""
    from tgp import kernels as K
    from tgp.nn import PANConv
    from tgp.poolers import PANPooling
    d = FI.draw("pan", seed, limits())
    case, report, fac = f"pan-public-{seed}", [], factor_of("pan")
    ex = FR.pan_exact(d)
    kept, native = ex["kept"], d["route"] == "native"
    ei, batch = mv(d["edge_index"]), mv(d["batch"])
    conv, pool = PANConv(FI.PAN_F, FI.PAN_F, d["filter_size"]).to(dev()), PANPooling(FI.PAN_F, ratio=0.5).to(dev())
    with torch.no_grad():
        for t, v in ((conv.weight, "weight"), (conv.lin.weight, "lin_w"), (conv.lin.bias, "lin_b"), (pool.p, "p"),
                     (pool.beta, "beta")):
            t.copy_(mv(d[v]))
    ints = {}

    def kernel():
        x = mv(d["x"]).requires_grad_(True)
        h, m = conv(x, ei, batch=batch)
        met = K.pan_record(m)
        assert met is not None and (met.frame is not None) == native, case
        res = pool(x=h, adj=m, batch=batch)
        order = torch.argsort(res.so.node_index)
        pooled = res.edge_index.coalesce()
        ints.update(index=m.indices(), kept=res.so.node_index[order], pooled_index=pooled.indices())
        outs = {"conv_out": h, "met_values": m.values(), "weight": res.so.weight[order],
                "x_pool": res.x[res.so.cluster_index[order]], "pooled_values": pooled.values()}
        return outs, {"x": x, "weight": conv.weight, "lin.weight": conv.lin.weight, "lin.bias": conv.lin.bias, "p": pool.p,
                      "beta": pool.beta}
    outs, _ = kernel()

    def oracle(dtype):
        return FR.pan_reference(d, dtype, ex)
    exact = {k: ex[k] for k in ("index", "kept", "pooled_index")}
    with torch.no_grad():
        r64, r32 = (_pan_split(d, ex, oracle(dt)[0], kept) for dt in (F64, F32))
    fails = forward_errors(case, dict(_pan_split(d, ex, {k: v.detach() for k, v in outs.items()}, kept), **ints),
                           dict(r64, **exact), r32, exact=set(exact), factor=fac, report=report)
    finish(case, fails, report)
    leaves = ["x", "weight", "lin.weight", "lin.bias", "p", "beta"]
    check_grads(case, kernel, oracle, leaves)
    if seed % 4 == 0:
        runs = []
        for _ in range(2):  # the same public call twice: equal bits, forward and backward
            o, lv = kernel()
            total = sum((v * mv(upstream(f"{case}/{k}", *v.shape))).sum() for k, v in o.items())
            runs.append([v.detach() for v in o.values()] + list(torch.autograd.grad(total, [lv[k] for k in leaves])))
        assert all(torch.equal(u, v) for u, v in zip(*runs)), case


# ===================================================================================================== EigenPooling
def _eig_check_modes(case, d, modes, fails, report, fac, skipped_over=()):
    """The modes [n, H] of a draw against the float64 ``cluster_modes``: the invariants of ``check_group_invariants`` for
    every group, the entries by the rule for the compared groups.  -> the groups left to the invariants alone."""
    import eigenpool_restatement as REG
    from test_gpu_eigenpool import check_group_invariants
    good, rest = FR.eigenpool_compared_groups(d)
    a = REG.dense_adjacency(d["edge_index"], d["edge_weight"], 0, d["n"])
    host = modes.cpu().double()
    for g, nodes in FR.eigenpool_groups(d):
        if g not in skipped_over:
            check_group_invariants(host[nodes], a[nodes][:, nodes], d["normalized"], d["H"])
    r64, r32 = (FR.eigenpool_operator_reference(d, dt)[0] for dt in (F64, F32))
    names = [f"modes[{g}]" for g in good if g not in skipped_over]
    got = {f"modes[{g}]": modes[mv(d["gid"] == g)] for g in good if g not in skipped_over}
    fails += forward_errors(case, got, {k: r64[k] for k in names}, r32, factor=fac, report=report)
    return rest


def _eig_reduce_x(d):
    x = mv(d["reduce_x"])
    if d["layout"] == "plain":
        return x
    base = torch.full((x.size(0), x.size(1) + 3), float("nan"), device=dev())
    base[:, 1:1 + x.size(1)] = x
    return base[:, 1:1 + x.size(1)]


def _rel_error(a, b):
    return float(torch.linalg.vector_norm(a.double() - b) / torch.linalg.vector_norm(b))


EIG_LEFT = {"op": {}, "public": {}}  # per layer and seed (groups left to the invariants, groups): the 5 % condition


def _eig_share(layer, seed, rest, d):
    """Asserts, once all 16 seeds of a layer have run in this process, that the groups it left to the invariants alone
    are at most 5 % of all groups (a run of fewer seeds checks nothing here: the CPU test holds the same share)."""
    EIG_LEFT[layer][seed] = (len(rest), len(FR.eigenpool_groups(d)))
    if len(EIG_LEFT[layer]) == len(SEEDS):
        left, total = (sum(v[i] for v in EIG_LEFT[layer].values()) for i in (0, 1))
        assert left <= 0.05 * total, (layer, left, total)


@pytest.mark.parametrize("seed", SEEDS)
def test_eigenpool_operators(seed):
    """``eigenpool_modes`` group by group (invariants always, entries where the float64 spectrum separates them; a group
    past the limit is flagged and left at zero), ``eigenpool_reduce`` and ``eigenpool_lift`` on a batch whose longest
    group sits at a kernel threshold among short and empty ones: by the rule, empty groups exact zero rows, the adjoint
    identity, and on one seed in four the ``max_len`` hint one class too low and one too high as well."""
    from tgp import kernels as K
    d = FI.draw("eigenpool", seed, limits())
    case, report, fac, fails = f"eigenpool-op-{seed}", [], factor_of("eigenpool"), []
    n, k, H, lim = d["n"], d["width"], d["H"], limits()["eigenpool_max_group_nodes"]
    ei, ew, gid = mv(d["edge_index"]), mv(d["edge_weight"]), mv(d["gid"]).to(torch.int32)
    by_src, groups = K.edge_group(ei, n), K.build_assign_index(mv(d["gid"]), 2 * k)
    sizes = torch.bincount(d["gid"], minlength=2 * k)
    over = (sizes > lim).nonzero().view(-1).tolist()

    def modes_of():
        return K.eigenpool_modes(by_src, ei[1], ew, gid, groups, H, min(int(sizes.max()), lim), d["normalized"])
    theta, st = modes_of()
    assert bool(st & K.EIG_OVER_LIMIT) == bool(over) and not st & K.EIG_ASYMMETRIC, (case, st)
    for g in over:
        assert float(theta[mv(d["gid"] == g)].abs().max()) == 0.0, case
    rest = _eig_check_modes(case, d, theta, fails, report, fac, skipped_over=over)
    # Reduce and Lift
    G, rH, longest = d["reduce_groups"], d["reduce_H"], d["longest"]
    rgid = mv(d["reduce_gid"])
    rgroups = K.build_assign_index(rgid, G)
    th, x, y = mv(d["theta"]), _eig_reduce_x(d), mv(d["reduce_y"])
    r64, r32 = (FR.eigenpool_operator_reference(d, dt)[0] for dt in (F64, F32))
    ref64, ref32 = ({k_: r[k_] for k_ in ("pool", "lift")} for r in (r64, r32))
    empty = (torch.tensor(d["rows"]) == 0).view(-1, 1).expand(G, rH * d["F"])
    hints = [longest] + ([FI.EIG_REDUCE_ONE_WAVE, FI.EIG_REDUCE_FOUR_WAVES, FI.EIG_REDUCE_FOUR_WAVES + 1] if d["hints"] else [])
    pools = {}
    for hint in dict.fromkeys(hints):  # (the hint picks the kernel, never the validity: every class within the bound)
        pools[hint] = K.eigenpool_reduce(th, rgroups, x, hint)
        got = {"pool": pools[hint], "lift": K.eigenpool_lift(th, rgid.to(torch.int32), y, G)}
        fails += forward_errors(f"{case}-hint{hint}", got, ref64, ref32, zeros={"pool": empty}, factor=fac, report=report)
    pool, lift = pools[longest], K.eigenpool_lift(th, rgid.to(torch.int32), y, G)
    # <Reduce(x), y> = <x, Lift(y)> to the bound times the sum of the terms' magnitudes
    lhs, rhs = float((pool.double() * y.double()).sum()), float((mv(d["reduce_x"]).double() * lift.double()).sum())
    scale = float((r64["pool"].abs() * d["reduce_y"].double().abs()).sum())
    bound = max(fac * max(_rel_error(r32["pool"], r64["pool"]), _rel_error(r32["lift"], r64["lift"])), 2e-6)
    if abs(lhs - rhs) > bound * scale:
        fails.append(f"{case}: adjoint identity off by {abs(lhs - rhs):.3e}, bound {bound * scale:.3e}")
    if seed % 4 == 0:
        again, st2 = modes_of()
        assert torch.equal(again, theta) and st2 == st, case
        assert torch.equal(K.eigenpool_reduce(th, rgroups, x, longest), pool), case
        assert torch.equal(K.eigenpool_lift(th, rgid.to(torch.int32), y, G), lift), case
    finish(case, fails, report)
    _eig_share("op", seed, rest, d)


@pytest.mark.parametrize("seed", SEEDS)
def test_eigenpool_public(seed):
    """``EigenPooling`` through ``labels=``: the compact pooling matrix's offsets, order and S exactly, its modes as in
    the operator layer (a group past the limit by the composed route: one ``eigh`` call per such group, none else),
    x_pool and the lifted rows of the compared groups and the pooled adjacency graph by graph, and the gradients of
    x_pool and of the lift to x."""
    from tgp.poolers import EigenPooling
    d = FI.draw("eigenpool", seed, limits())
    case, report, fac, fails = f"eigenpool-public-{seed}", [], factor_of("eigenpool"), []
    lim, k = limits()["eigenpool_max_group_nodes"], d["width"]
    over = int((torch.bincount(d["gid"], minlength=2 * k) > lim).sum())
    good = torch.tensor(FR.eigenpool_compared_groups(d)[0])
    rows = torch.isin(d["gid"], good)
    pooler = EigenPooling(k=k, num_modes=d["H"], normalized=d["normalized"])
    ei, ew, batch, labels = mv(d["edge_index"]), mv(d["edge_weight"]), mv(d["batch"]), mv(d["labels"])
    state = {}

    def kernel():
        x = mv(d["x"]).requires_grad_(True)
        with _Calls(torch.linalg, "eigh") as calls:
            out = pooler(x=x, adj=ei, edge_weight=ew, batch=batch, labels=labels)
        assert calls.count["eigh"] == over, (case, calls.count, over)  # the composed route for the groups past the limit alone
        lift = pooler(x=out.x, so=out.so, batch=out.so.batch, lifting=True)
        state.update(out=out)
        return {"x_pool": out.x.reshape(2 * k, -1)[mv(good)], "lift": lift[mv(rows)], "adj": out.edge_index}, {"x": x}
    outs, _ = kernel()
    so = state["out"].so
    exact = FR.eigenpool_exact(d)
    ints = {"theta_ptr": so.theta_ptr, "theta_perm": so.theta_perm, "s": so.s}
    rest = _eig_check_modes(case, d, so.theta_modes, fails, report, fac)
    with torch.no_grad():
        r64, r32 = (FR.eigenpool_reference(d, dt)[0] for dt in (F64, F32))

    def by_graph(o):  # x_pool's rows by the graph of their group, the lifted rows by their node's graph, adj per graph
        res = dict(o)
        for b in range(2):
            res[f"x_pool[{b}]"] = o["x_pool"][(good // k == b).to(o["x_pool"].device)]
            res[f"lift[{b}]"] = o["lift"][(d["batch"][rows] == b).to(o["lift"].device)]
            res[f"adj[{b}]"] = o["adj"][b]
        return res
    fails += forward_errors(case, dict(by_graph({k_: v.detach() for k_, v in outs.items()}), **ints),
                            dict(by_graph(r64), **exact), by_graph(r32), exact=set(exact), factor=fac, report=report)
    finish(case, fails, report)

    def paths(fn):  # (the pooled adjacency does not depend on x)
        def run(*a):
            o, lv = fn(*a)
            return {k_: v for k_, v in o.items() if k_ != "adj"}, lv
        return run
    check_grads(case, paths(kernel), paths(lambda dt: FR.eigenpool_reference(d, dt)), ["x"])
    if seed % 4 == 0:
        again, _ = kernel()
        assert all(torch.equal(v.detach(), again[k_].detach()) for k_, v in outs.items()), case
    _eig_share("public", seed, rest, d)
