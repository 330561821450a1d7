"""Non-finite inputs through the older operator families, against the CPU oracle on the same inputs.

The reference is plain torch: a NaN propagates through ``clamp``, ``max``, ``amax`` / ``amin``, ``norm`` and
``softmax``.  tests/test_oracle_golden.py pins the oracle to the reference's own non-finite results
(tests/golden/golden_nonfinite_v1.pt); here every kernel route of sparse Connect, sparse Reduce, dense Reduce + Connect,
the dense post-processing, the fused losses, TopK and MLPSelect must agree with that oracle: equal NaN masks, equal
infinities with sign, the finite rest at the tolerance the family's own test file uses (``TOL`` of test_gpu_fuzz.py,
``_close64`` of test_gpu_dense_pool.py), integer outputs bit for bit (tests/nonfinite.py).  Graclus has no reference
matching to compare with (torch_cluster's is randomised): its own contract is asserted.

Finite entries have magnitude in [0.05, 2] and the shapes are small, so no finite sum comes near overflow and the
position of every non-finite output is independent of the summation order.  Each test asserts that on the CPU: the
oracle's result on the un-planted input is all finite.  Each test also asserts the route it meant to take.
"""
import itertools

import pytest
import torch

import tgp_oracle as O
from nonfinite import KINDS, assert_same_nonfinite, plant
from test_gpu_dense_pool import _close64, _oracle64
from test_gpu_fuzz import TOL

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
OPS = ["sum", "mean", "min", "max", "mul"]
DTYPES = [torch.float32, torch.float64]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _vals(shape, g, dtype=torch.float32, signed=False):
    """Finite entries of magnitude in [0.05, 2]."""
    v = torch.rand(shape, generator=g, dtype=torch.float64) * 1.95 + 0.05
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return v.to(dtype)


def _all_finite(*ts):
    return all(t is None or not t.is_floating_point() or bool(torch.isfinite(t).all()) for t in ts)


def _same(got, want, what, dtype=torch.float32):
    """``assert_same_nonfinite`` at the family's tolerance: TOL for float32, _close64 for float64."""
    if want is None:
        assert got is None, what
        return
    if want.is_floating_point():
        assert got.dtype == dtype, f"{what}: {got.dtype}"
        if dtype == torch.float64:
            return assert_same_nonfinite(got, want, what, close=_close64)
        return assert_same_nonfinite(got, want.to(dtype), what, **TOL)
    assert_same_nonfinite(got, want, what)


class _Cases(list):
    """Every planted case of a test is compared, whatever the earlier ones gave; ``done`` raises with all that differ."""

    def same(self, *a, **k):
        try:
            _same(*a, **k)
        except AssertionError as exc:
            self.append(str(exc).splitlines()[0])

    def equal_index(self, got, want, what):
        if got.shape != want.shape or not torch.equal(got.cpu(), want):
            self.append(f"{what}: edge_index differs: {got.size(1)} entries, the reference has {want.size(1)}")
            return False
        return True

    def done(self):
        assert not self, f"{len(self)} cases differ from the reference:\n" + "\n".join(self)


def _oracle(dtype, fn, *a, **k):
    return _oracle64(fn, *a, **k) if dtype == torch.float64 else fn(*a, **k)


def _plant_at(t, idx, kind, g):
    """``plant`` on the entries ``idx`` of the vector ``t`` (a NaN / an infinity on the first of them, the pair on the
    first and a drawn other one); returns the planted positions in ``t``."""
    idx = torch.as_tensor(idx, dtype=torch.long)
    sub = t[idx].clone()
    pos = plant(sub, kind, "first", g, axis=0)
    t[idx] = sub
    return idx[pos[:, 0]]


# ====================================================================================== sparse Connect: coalesce
def _connect_problem(n):
    """A sorted batch ([4, 3] nodes for n = 7, three graphs of 50 for n = 150), a row-sorted directed edge list with
    duplicates and self loops (E <= 700), and a clustering -- singles and one pair per graph for n = 7; pairs for
    n = 150, with ONE hub supernode of 30 nodes whose row of 120 raw entries takes the long-row path of the fused route.
    ``targets``: entry lists to plant into -- "single" (a group of one; two of them in one supernode row, so that a pair
    meets in the row's degree), "dup" (a group of at least three entries), "hub" (a group of at least two inside the hub
    row; n = 150)."""
    for seed in range(64):
        g = _gen(100 * n + seed)
        sizes = [4, 3] if n == 7 else [50, 50, 50]
        batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
        start = torch.cumsum(torch.tensor(sizes), 0) - torch.tensor(sizes)
        deg = 3 if n == 7 else 4
        src = torch.arange(n).repeat_interleave(deg)
        dst = start[batch[src]] + (torch.rand(src.numel(), generator=g) * torch.tensor(sizes)[batch[src]]).long()
        ei = torch.stack([src, dst])  # rows ascending, columns in drawing order, duplicates and loops as they come
        cluster, k, hub = torch.empty(n, dtype=torch.long), 0, None
        for b, (s0, nb) in enumerate(zip(start.tolist(), sizes)):
            first = 0
            if n == 150 and b == 0:
                cluster[s0:s0 + 30], hub, k, first = k, k, k + 1, 30
            local = torch.arange(nb - first) // 2 if n == 150 else torch.tensor([0, 1, 1, 2][:nb])
            cluster[s0 + first:s0 + nb] = k + local
            k += int(local.max()) + 1
        bp = torch.empty(k, dtype=torch.long)
        bp[cluster] = batch
        cr, cc = cluster[ei[0]], cluster[ei[1]]
        key = cr * k + cc
        size = torch.bincount(key, minlength=k * k)[key]
        off = cr != cc  # self loops of the pooled graph fall to remove_self_loops: plant where the flag cannot hide it
        singles = (off & (size == 1)).nonzero().view(-1)
        targets = {}
        for e in singles.tolist():
            mates = [m for m in singles.tolist() if m != e and cr[m] == cr[e]]
            if mates:
                targets["single"] = [e, mates[0]]
                break
        dups = (off & (size >= 3) & (cr != (hub if hub is not None else -1))).nonzero().view(-1)
        if dups.numel():
            targets["dup"] = (key == key[dups[0]]).nonzero().view(-1).tolist()
        if hub is not None:
            hubs = (off & (size >= 2) & (cr == hub)).nonzero().view(-1)
            if hubs.numel():
                targets["hub"] = (key == key[hubs[0]]).nonzero().view(-1).tolist()
        if len(targets) == (3 if n == 150 else 2):
            assert ei.size(1) <= 700
            return dict(n=n, k=k, ei=ei, cluster=cluster, batch=batch, bp=bp, hub=hub, targets=targets,
                        ew=_vals((ei.size(1),), g, torch.float64), x=_vals((n, 8), g), sizes=sizes)
    raise AssertionError("no seed gives every target group")


_PROBLEMS = {}


def _problem(n):
    if n not in _PROBLEMS:
        _PROBLEMS[n] = _connect_problem(n)
    return _PROBLEMS[n]


def _connect_ref(p, ew, op, flags, dtype):
    rsl, dn, ewn = flags
    return _oracle(dtype, O.sparse_connect, p["ei"], ew.to(dtype), torch.arange(p["n"]), p["cluster"], p["n"], p["k"],
                   remove_self_loops=rsl, reduce_op=op, edge_weight_norm=ewn, batch_pooled=p["bp"], degree_norm=dn)


def _connect_cases(p):
    """(tag, kind, planted weights, planted positions): every kind in a group of one and in a group with duplicates,
    and a NaN inside the hub row."""
    for where, kind in itertools.product(("single", "dup"), KINDS):
        ew = p["ew"].clone()
        idx = p["targets"][where]
        pos = _plant_at(ew, idx if (kind == "inf_pair" or where == "dup") else idx[:1], kind, _gen(5))
        yield f"{kind} in a {where} group", kind, ew, pos
    if "hub" in p["targets"]:
        ew = p["ew"].clone()
        yield "nan in the hub row", "nan", ew, _plant_at(ew, p["targets"]["hub"], "nan", _gen(6))


PLAIN, ALL_FLAGS = (False, False, False), (True, True, True)


def _run_connect(p, op, dtype, dev, coalesce):
    """``coalesce(ei, ew, remove_self_loops)`` -> the pooled list of one route; both flag sets, every plant."""
    from tgp.utils.ops import postprocess_adj_pool_sparse
    eid, bpd = p["ei"].to(dev), p["bp"].to(dev)
    cases = _Cases()
    for flags in (PLAIN, ALL_FLAGS):
        clean = _connect_ref(p, p["ew"], op, flags, dtype)
        assert _all_finite(*clean), "the un-planted reference must be finite"
        for tag, kind, ew, pos in _connect_cases(p):
            ref_ei, ref_ew = _connect_ref(p, ew, op, flags, dtype)
            changed = (ref_ei.shape != clean[0].shape or not torch.equal(ref_ei, clean[0])
                       or not bool(torch.isfinite(ref_ew).all()))
            if kind in ("nan", "inf_pair"):  # (an infinity of the losing sign leaves a min / max as it was)
                assert changed, f"{tag}: the plant at {pos.tolist()} leaves the reference as it was"
            got_ei, got_ew = coalesce(eid, ew.to(dtype).to(dev), flags[0])
            if flags is ALL_FLAGS:
                got_ei, got_ew = postprocess_adj_pool_sparse(got_ei, got_ew, num_nodes=p["k"], remove_self_loops=True,
                                                             degree_norm=True, edge_weight_norm=True, batch_pooled=bpd)
            what = f"n={p['n']} {op} {dtype} flags={flags} {tag}"
            if cases.equal_index(got_ei, ref_ei, what):
                cases.same(got_ew, ref_ew, what, dtype)
    cases.done()


@pytest.mark.parametrize("n", [7, 150])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("route", ["general", "fused", "staged"])
def test_coalesce_routes(dev, route, op, dtype, n):
    """``tgp.kernels.coalesce_edges`` forced onto one route (the C entry points of csrc/sparse_connect.hip and
    coalesce_rows.hip) against ``O.sparse_connect``.  float64 weights have the staged and the general route."""
    from tgp import kernels
    p = _problem(n)
    cl = p["cluster"].to(dev)
    if dtype == torch.float64 and route == "fused":
        with pytest.raises(RuntimeError, match="float64 edge weights take"):
            kernels.coalesce_edges(p["ei"].to(dev), p["ew"].to(dev), cl, p["k"], op, True, route=route)
        return
    if route == "fused" and n == 150:  # the hub row is a long row of the fused kernel (65 .. 1024 raw entries)
        row = (p["cluster"][p["ei"][0]] == p["hub"]).sum()
        assert 64 < int(row) <= 1024

    def coalesce(ei, ew, rsl):  # (a forced route raises if it declines)
        return kernels.coalesce_edges(ei, ew, cl, p["k"], op, rsl, route=route)
    _run_connect(p, op, dtype, dev, coalesce)


@pytest.mark.parametrize("n", [7, 150])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("op", OPS)
def test_sparse_connect_wrapper(dev, op, dtype, n):
    """The public ``SparseConnect`` (the route the library picks), plain and with remove_self_loops + degree_norm +
    edge_weight_norm."""
    from tgp.connect import SparseConnect
    from tgp.select import SelectOutput
    p = _problem(n)
    so = SelectOutput(cluster_index=p["cluster"].to(dev), num_nodes=n, num_supernodes=p["k"])
    eid, bpd = p["ei"].to(dev), p["bp"].to(dev)
    cases = _Cases()
    for flags in (PLAIN, ALL_FLAGS):
        conn = SparseConnect(reduce_op=op, remove_self_loops=flags[0], degree_norm=flags[1], edge_weight_norm=flags[2])
        assert _all_finite(*_connect_ref(p, p["ew"], op, flags, dtype))
        for tag, kind, ew, pos in _connect_cases(p):
            ref_ei, ref_ew = _connect_ref(p, ew, op, flags, dtype)
            got_ei, got_ew = conn(eid, so, edge_weight=ew.to(dtype).to(dev), batch_pooled=bpd)
            what = f"n={n} {op} {dtype} flags={flags} {tag}"
            if cases.equal_index(got_ei, ref_ei, what):
                cases.same(got_ew, ref_ew, what, dtype)
    cases.done()


@pytest.mark.parametrize("n", [7, 150])
@pytest.mark.parametrize("op", OPS)
def test_small_graph_one_launch_connect(dev, op, n):
    """The one-launch Reduce + Connect of a sorted batch of small graphs (csrc/sparse_pool_small.hip) through
    ``pooler.reduce_connect``: it must take the call (not None), and x', batch', edge_index' and the weights must be the
    oracle's."""
    from tgp import kernels
    from tgp.poolers import get_pooler
    from tgp.select import SelectOutput
    p = _problem(n)
    assert max(p["sizes"]) <= kernels.sparse_pool_small_max_graph_nodes() and len(p["sizes"]) >= 2
    xd, eid, bd = p["x"].to(dev), p["ei"].to(dev), p["batch"].to(dev)
    ref_x = O.reduce_sparse(p["x"], torch.arange(n), p["cluster"], torch.ones(n), p["k"])
    cases = _Cases()
    for flags in (PLAIN, ALL_FLAGS):
        pooler = get_pooler("graclus", connect_red_op=op, remove_self_loops=flags[0], degree_norm=flags[1],
                            edge_weight_norm=flags[2]).to(dev).eval()
        assert _all_finite(*_connect_ref(p, p["ew"], op, flags, torch.float32))
        for tag, kind, ew, pos in _connect_cases(p):
            so = SelectOutput(cluster_index=p["cluster"].to(dev), num_nodes=n, num_supernodes=p["k"])
            with torch.no_grad():
                got = pooler.reduce_connect(xd, eid, ew.float().to(dev), so, bd)
            assert got is not None, "the one-launch kernel declined a sorted batch of small graphs"
            ref_ei, ref_ew = _connect_ref(p, ew, op, flags, torch.float32)
            what = f"n={n} {op} flags={flags} {tag}"
            if cases.equal_index(got[2], ref_ei, what):
                cases.same(got[3], ref_ew, what)
            assert torch.equal(got[1].cpu(), p["bp"])
            cases.same(got[0], ref_x, what + " x_pool")
    cases.done()


# ====================================================================================== sparse Connect: subgraph
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_subgraph_connect(dev, dtype):
    """A strict subset of the nodes (``O.sparse_connect``'s first branch): a NaN on a kept edge is removed by the eps
    filter, an infinity on a kept edge stays, a NaN on a dropped edge changes nothing, and ``degree_norm`` with both
    infinities in one row makes that row's and that column's entries NaN."""
    from tgp.connect import sparse_connect
    g = _gen(31)
    n, e = 150, 700
    ei = torch.stack([torch.sort(torch.randint(0, n, (e,), generator=g))[0], torch.randint(0, n, (e,), generator=g)])
    ei = ei[:, ei[0] != ei[1]]
    kept = torch.sort(torch.randperm(n, generator=g)[:n // 2])[0]
    kk = kept.numel()
    is_kept = torch.zeros(n, dtype=torch.bool)
    is_kept[kept] = True
    inside = (is_kept[ei[0]] & is_kept[ei[1]]).nonzero().view(-1)
    outside = (~is_kept[ei[0]]).nonzero().view(-1)
    rows = ei[0][inside]
    twice = [int(r) for r in rows.unique() if int((rows == r).sum()) >= 3][0]  # a kept row with three kept entries
    in_row = inside[rows == twice]
    ew0 = _vals((ei.size(1),), g, torch.float64)
    bp = torch.sort(torch.randint(0, 2, (kk,), generator=g))[0]
    cases = _Cases()

    def run(ew, **flags):
        ref = _oracle(dtype, O.sparse_connect, ei, ew.to(dtype), kept, torch.arange(kk), n, kk, batch_pooled=bp, **flags)
        got = sparse_connect(ei.to(dev), ew.to(dtype).to(dev), node_index=kept.to(dev),
                             cluster_index=torch.arange(kk, device=dev), num_nodes=n, num_supernodes=kk,
                             batch_pooled=bp.to(dev), **flags)
        if cases.equal_index(got[0], ref[0], f"subgraph {dtype} {flags}"):
            cases.same(got[1], ref[1], f"subgraph {dtype} {flags}", dtype)
        return ref

    clean = run(ew0)
    assert _all_finite(*clean)
    ew = ew0.clone()
    ew[inside[0]] = NAN
    assert run(ew)[0].size(1) == clean[0].size(1) - 1            # removed by |w| > eps
    for v in (INF, -INF):
        ew = ew0.clone()
        ew[inside[1]] = v
        ref = run(ew)
        assert ref[0].size(1) == clean[0].size(1) and int(torch.isinf(ref[1]).sum()) == 1  # it stays
    ew = ew0.clone()
    ew[outside[0]] = NAN
    ref = run(ew)
    assert torch.equal(ref[0], clean[0]) and torch.equal(ref[1], clean[1])                  # a dropped edge
    ew = ew0.clone()
    ew[in_row[0]], ew[in_row[1]] = INF, -INF
    for flags in (dict(degree_norm=True), dict(degree_norm=True, edge_weight_norm=True, remove_self_loops=False)):
        assert _all_finite(*run(ew0, **flags))
        ref = run(ew, **flags)
        assert bool(torch.isnan(ref[1]).any())
    cases.done()


# ============================================================================================== sparse Reduce
def _reduce_problem(f, dtype, seed, topk):
    g = _gen(seed)
    n = 150
    x = _vals((n, f), g, dtype, signed=True)
    if topk:  # one node per supernode, a strict subset
        k = 70
        ni = torch.sort(torch.randperm(n, generator=g)[:k])[0]
        ci = torch.randperm(k, generator=g)
    else:     # clusters of several nodes over two thirds of the nodes: the rest belongs to no supernode
        k = 33
        ni = torch.sort(torch.randperm(n, generator=g)[:100])[0]
        ci = torch.randint(0, k, (100,), generator=g)
    w = _vals((ni.numel(),), g, dtype, signed=True)
    free = torch.ones(n, dtype=torch.bool)
    free[ni] = False
    return n, k, x, ni, ci, w, free.nonzero().view(-1)


@pytest.mark.parametrize("route", ["vector", "scalar", "f64"])
def test_sparse_reduce(dev, route):
    """``BaseReduce`` on a sparse assignment (csrc/sparse_reduce.hip; ``tgp_reduce_sparse_f64``): F = 32 (16-byte rows,
    the vector loads) and F = 7 (scalar loads).  A plant in ``x`` at a kept node shows in its supernode's row and nowhere
    else; at a node no supernode owns it must not leak; a plant in ``weight``; a weight of exactly 0 against an infinite
    ``x`` gives NaN, as the reference's product does."""
    from tgp.reduce import BaseReduce
    from tgp.select import SelectOutput
    dtype = torch.float64 if route == "f64" else torch.float32
    f = 7 if route == "scalar" else 32
    n, k, x0, ni, ci, w0, free = _reduce_problem(f, dtype, 41, topk=False)
    batch = torch.zeros(n, dtype=torch.long)
    cases = _Cases()

    def run(x, w, what):
        so = SelectOutput(node_index=ni.to(dev), cluster_index=ci.to(dev), num_nodes=n, num_supernodes=k, weight=w.to(dev))
        xd = x.to(dev)
        if route == "vector":
            assert xd.data_ptr() % 16 == 0 and f % 4 == 0
        got, bp = BaseReduce()(xd, so, batch=batch.to(dev))
        ref = _oracle(dtype, O.reduce_sparse, x, so.node_index.cpu(), so.cluster_index.cpu(), so.weight.cpu(), k)
        cases.same(got, ref, f"{route} {what}", dtype)
        assert torch.equal(bp.cpu(), O.reduce_batch_sparse(batch, so.node_index.cpu(), so.cluster_index.cpu(), k))
        return ref

    assert _all_finite(run(x0, w0, "clean"))
    g = _gen(7)
    for kind in KINDS:
        for where in ("first", "last", "tail", "tile_row"):
            x = x0.clone()
            rows = x[ni]  # the kept nodes' rows
            pos = plant(rows, kind, where, g)
            x[ni] = rows
            ref = run(x, w0, f"x {kind} {where}")
            hit = torch.unique(ci[pos[:, 0]])
            bad = (~torch.isfinite(ref)).any(1).nonzero().view(-1)
            assert torch.equal(bad, hit), (kind, where)  # its supernode's row, no other row
        x = x0.clone()
        rows = x[free]
        plant(rows, kind, "per_graph", g, ptr=torch.tensor([0, free.numel() // 2, free.numel()]))
        x[free] = rows
        assert _all_finite(run(x, w0, f"x {kind} at nodes without a supernode"))
        w = w0.clone()
        members = (ci == torch.bincount(ci, minlength=k).argmax()).nonzero().view(-1)  # the largest supernode
        _plant_at(w, members.tolist(), kind, g)
        ref = run(x0, w, f"weight {kind}")
        assert not _all_finite(ref)
    x, w = x0.clone(), w0.clone()
    x[ni[3], 1], w[3] = INF, 0.0
    ref = run(x, w, "0 * inf")
    assert bool(torch.isnan(ref[ci[3], 1]))
    cases.done()


def test_sparse_reduce_packed_index_from_the_topk_selector(dev, monkeypatch):
    """The packed one-to-one index the TopK selector hands over (``tgp_reduce_one_to_one_f32``: F % 4 == 0, F >= 32):
    the kept NaN / infinite score multiplies its row, a NaN feature of a kept node stays in its row."""
    from tgp import kernels
    from tgp.reduce import BaseReduce
    from tgp.select import TopkSelect
    g = _gen(43)
    n, f = 150, 32
    x0 = _vals((n, f), g, signed=True)
    score0 = _vals((n,), g, signed=True)
    batch = torch.repeat_interleave(torch.arange(3), 50)
    calls, lib = [], kernels.N.lib()
    real = lib.tgp_reduce_one_to_one_f32
    monkeypatch.setattr(lib, "tgp_reduce_one_to_one_f32", lambda *a_: (calls.append(1), real(*a_))[1])
    for kind in KINDS:
        score, x = score0.clone(), x0.clone()
        plant(score, kind, "per_graph", g, ptr=torch.tensor([0, 50, 100, 150]))
        plant(x, "nan", "tile_row", g)
        sel = TopkSelect(in_channels=None, ratio=0.5, act="linear").to(dev)
        so = sel(score.view(-1, 1).to(dev), batch=batch.to(dev))
        assert so.assign_index().pack is not None, "the selector left no packed index"
        calls.clear()
        got, _ = BaseReduce()(x.to(dev), so, batch=batch.to(dev))
        assert calls == [1], "the Reduce did not take the packed-index kernel"
        ni, ci, w = so.node_index.cpu(), so.cluster_index.cpu(), so.weight.cpu()
        r_ni, r_ci, r_w = O.topk_select(score, None, 0.5, batch, act="linear")
        assert torch.equal(ni, r_ni) and torch.equal(ci, r_ci)
        _same(w, r_w, f"{kind}: weights of S")
        clean = O.reduce_sparse(x0, r_ni, r_ci, torch.ones_like(r_w), r_ni.numel())
        assert _all_finite(clean)
        _same(got, O.reduce_sparse(x, r_ni, r_ci, r_w, r_ni.numel()), f"packed index, {kind} score")


# ====================================================================================== dense Reduce + Connect
def _dense_problem(B, N, K, F, dtype, seed):
    g = _gen(seed)
    s = torch.softmax(torch.randn(B, N, K, generator=g, dtype=torch.float64), -1).to(dtype)
    a = ((torch.rand(B, N, N, generator=g) < 0.3).double() * _vals((B, N, N), g, torch.float64)).to(dtype)
    x = _vals((B, N, F), g, dtype, signed=True)
    return s, a, x


def _dense_plants(s0, a0, x0, g):
    """(what, s, a, x): one row of S, one entry of X, one entry of A -- all in graph 0 -- for every kind."""
    for kind in KINDS:
        s = s0.clone()
        row = s[0, min(63, s.size(1) - 1)]  # the last row of the first tile
        row.fill_(NAN if kind == "nan" else INF if kind != "-inf" else -INF)
        if kind == "inf_pair":
            row[1::2] = -INF
        yield f"{kind} row of S", s, a0, x0
        x = x0.clone()
        plant(x[0], kind, "tail", g, axis=-2)
        yield f"{kind} in X", s0, a0, x
        a = a0.clone()
        plant(a[0], kind, "tile_row", g)
        yield f"{kind} in A", s0, a, x0


def _check_dense(cases, got, s, a, x, what, dtype, flags=(True, True, True, False)):
    """x_pool, raw S^T A S and the post-processed adjacency against the oracle; graph 1 stays finite."""
    ref_x = _oracle(dtype, O.reduce_dense, s, x)
    ref_raw = _oracle(dtype, O.dense_connect, s, a)
    ref_post = _oracle(dtype, O.postprocess_dense, ref_raw, *flags)
    for name, g_, r_ in (("x_pool", got[0], ref_x), ("raw", got[1], ref_raw), ("adj_pool", got[2], ref_post)):
        if g_ is not None:
            cases.same(g_, r_, f"{what}: {name}", dtype)
    assert _all_finite(ref_x[1], ref_raw[1], ref_post[1]), f"{what}: a plant in graph 0 reached graph 1 of the reference"
    for g_ in got[:3]:
        if not (g_ is None or _all_finite(g_[1].cpu())):
            cases.append(f"{what}: a plant in graph 0 reached graph 1")


DENSE_ROUTES = {  # B, N, K, F, dtype: the kernel each shape takes is asserted from the library's own predicate
    "gemm": (2, 150, 20, 9, torch.float32),
    "gemm_k72": (2, 150, 72, 9, torch.float32),
    "small": (64, 40, 12, 9, torch.float32),
    "f64": (2, 70, 5, 3, torch.float64),
}


@pytest.mark.parametrize("route", sorted(DENSE_ROUTES))
def test_dense_reduce_connect_fused_call(dev, route):
    """``tgp.kernels.dense_pool`` (the C entry points tgp_dense_pool_f32 / _f64): the tiled MFMA route, the
    one-wave-per-graph kernel of a batch of small graphs, and the float64 route."""
    from tgp import kernels as K
    B, N, Kc, F, dtype = DENSE_ROUTES[route]
    assert K.dense_pool_is_small(B, N, Kc, F) == (route == "small")
    s0, a0, x0 = _dense_problem(B, N, Kc, F, dtype, 51)
    flags = K.dense_flags(True, True, True, False)

    cases = _Cases()

    def run(s, a, x, what):
        got = K.dense_pool(s.to(dev), a.to(dev), x.to(dev), flags, want_raw=True)
        _check_dense(cases, got, s, a, x, f"{route} {what}", dtype)
    assert _all_finite(_oracle(dtype, O.postprocess_dense, _oracle(dtype, O.dense_connect, s0, a0), True, True, True, False))
    run(s0, a0, x0, "clean")
    for what, s, a, x in _dense_plants(s0, a0, x0, _gen(8)):
        run(s, a, x, what)
    cases.done()


@pytest.mark.parametrize("route", sorted(DENSE_ROUTES))
def test_dense_reduce_connect_wrappers(dev, route):
    """The public ``BaseReduce`` and ``DenseConnect`` on padded tensors, with a mask: a plant in a padded row of X, of
    A and of S (0 * NaN is NaN in the reference's products)."""
    from tgp.connect import DenseConnect
    from tgp.reduce import BaseReduce
    from tgp.select import SelectOutput
    B, N, Kc, F, dtype = DENSE_ROUTES[route]
    s0, a0, x0 = _dense_problem(B, N, Kc, F, dtype, 52)
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[:, N - 3:] = False
    s0, x0 = s0 * mask.unsqueeze(-1), x0 * mask.unsqueeze(-1)
    a0 = a0 * mask.unsqueeze(1) * mask.unsqueeze(2)
    conn = DenseConnect(True, True, True, False)
    cases = _Cases()

    def run(s, a, x, what):
        so = SelectOutput(s=s.to(dev))
        xp, _ = BaseReduce()(x.to(dev), so)
        raw = conn.dense_connect(adj=a.to(dev), s=s.to(dev))
        post, _ = conn(a.to(dev), so)
        _check_dense(cases, (xp, raw, post), s, a, x, f"{route} wrappers {what}", dtype)
    run(s0, a0, x0, "clean")
    for what, s, a, x in _dense_plants(s0, a0, x0, _gen(9)):
        run(s, a, x, what)
    for kind in ("nan", "+inf"):
        v = NAN if kind == "nan" else INF
        x = x0.clone()
        x[0, N - 1, 1] = v
        run(s0, a0, x, f"{kind} in a padded row of X")
        a = a0.clone()
        a[0, N - 2, 3] = v
        run(s0, a, x0, f"{kind} in a padded row of A")
        s = s0.clone()
        s[0, N - 1, 0] = v
        run(s, a0, x0, f"{kind} in a padded row of S")
    cases.done()


def test_dense_connect_unpadded_rows(dev, monkeypatch):
    """The un-padded form (sparse A, S [N, K], a batch vector): ``DenseConnect`` runs a CSR SpMM and one segment GEMM
    over all graphs, ``BaseReduce`` the segment GEMM; float32 and float64."""
    from tgp import functions as Fn
    from tgp.connect import DenseConnect
    from tgp.reduce import BaseReduce
    from tgp.select import SelectOutput
    g = _gen(53)
    sizes = torch.tensor([70, 33])
    n, Kc, F = int(sizes.sum()), 7, 5
    batch = torch.repeat_interleave(torch.arange(2), sizes)
    key = torch.unique(torch.randint(0, n * n, (600,), generator=g))
    ei = torch.stack([key // n, key % n])
    ei = ei[:, batch[ei[0]] == batch[ei[1]]]
    calls = []
    real = Fn.segment_gemm_tn
    monkeypatch.setattr(Fn, "segment_gemm_tn", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1])
    cases = _Cases()
    for dtype in DTYPES:
        s0 = torch.softmax(torch.randn(n, Kc, generator=g, dtype=torch.float64), -1).to(dtype)
        x0 = _vals((n, F), g, dtype, signed=True)
        w0 = _vals((ei.size(1),), g, dtype)
        conn = DenseConnect(remove_self_loops=True, degree_norm=True, adj_transpose=False)

        def run(s, x, w, what):
            so = SelectOutput(s=s.to(dev), batch=batch.to(dev))
            calls.clear()
            post, _ = conn(ei.to(dev), so, edge_weight=w.to(dev), batch=batch.to(dev))
            assert calls, "the segment GEMM of the un-padded route did not run"
            xp, _ = BaseReduce()(x.to(dev), so, batch=batch.to(dev), return_batched=True)
            raw = _oracle(dtype, O.dense_connect_unbatched, ei, w, batch, s)
            ref = _oracle(dtype, O.postprocess_dense, raw, True, True, False, False)
            ref_x = _oracle(dtype, O.reduce_dense, s, x, batch, True)
            cases.same(post, ref, f"rows {dtype} {what}: adj_pool", dtype)
            cases.same(xp, ref_x, f"rows {dtype} {what}: x_pool", dtype)
            return ref, ref_x
        assert _all_finite(*run(s0, x0, w0, "clean"))
        for kind in KINDS:
            s = s0.clone()
            plant(s[:70], kind, "tile_row", g)
            ref, ref_x = run(s, x0, w0, f"{kind} in S")
            assert not _all_finite(ref[0]) and _all_finite(ref[1], ref_x[1])  # graph 0 only
            x = x0.clone()
            plant(x[:70], kind, "tail", g, axis=0)
            ref, ref_x = run(s0, x, w0, f"{kind} in X")
            assert not _all_finite(ref_x[0]) and _all_finite(ref_x[1], ref)
            w = w0.clone()
            rows0 = ei[0][batch[ei[0]] == 0]
            _plant_at(w, (ei[0] == rows0.mode().values).nonzero().view(-1).tolist(), kind, g)  # entries of one row of A
            ref, _ = run(s0, x0, w, f"{kind} in A")
            assert not _all_finite(ref[0]) and _all_finite(ref[1])
    cases.done()


# ========================================================================================= dense post-processing
POST_K = [7, 20, 40, 128, 200, 513]  # post_tiny (<= 32), post_small (<= 64), the LDS kernel (<= 176), the three-kernel route


def _post_inputs(K, dtype):
    """name -> [3, K, K]: graph 0 carries the plant, graph 1 is finite, graph 2 is all zero where the name says so."""
    g = _gen(600 + K)
    base = _vals((3, K, K), g, dtype) * (torch.rand(3, K, K, generator=g) < 0.6)
    out = {}
    for where in ("first", "last", "tail", "tile_row"):
        a = base.clone()
        plant(a[0], "nan", where, g)
        out[f"a NaN entry ({where})"] = a
    a = base.clone()
    plant(a[0], "inf_pair", "tile_row", g)
    out["both infinities in one row"] = a
    a = base.clone()
    plant(a[0], "inf_pair", "tail", g, axis=-2)
    out["both infinities in one column"] = a
    a = base.clone()
    a[0, K // 2] = -a[0, K // 2] - 0.01
    out["a row with a negative sum"] = a
    a = base.clone()
    a[2] = 0
    out["an all-zero graph"] = a
    a = base.clone()
    plant(a[0], "+inf", "last", g)
    out["an infinite entry"] = a
    return base, out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("K", POST_K)
def test_postprocess_dense(dev, K, dtype):
    """``postprocess_adj_pool_dense`` on [3, K, K], all 16 flag combinations, at the cluster counts that select the
    variants of csrc/dense_post.h (and their float64 twins) against ``O.postprocess_dense``."""
    from tgp.utils.ops import postprocess_adj_pool_dense
    base, inputs = _post_inputs(K, dtype)
    combos = list(itertools.product((True, False), repeat=4))
    for flags in combos:
        assert _all_finite(_oracle(dtype, O.postprocess_dense, base, *flags))
    cases = _Cases()
    for name, a in inputs.items():
        ad = a.to(dev)
        for flags in combos:
            got = postprocess_adj_pool_dense(ad.clone(), *flags)
            ref = _oracle(dtype, O.postprocess_dense, a, *flags)
            cases.same(got, ref, f"K={K} {dtype} rsl/dn/at/ewn={flags} {name}", dtype)
            assert _all_finite(ref[1]) and _all_finite(got[1].cpu())  # the plant stays in its graph
    cases.done()


def test_postprocess_dense_entry_point(dev):
    """The same through the C entry point behind ``tgp.kernels.dense_pool`` with S = I: raw = A, post-processed in the
    fused call."""
    from tgp import kernels as K_
    Kc = 20
    base, inputs = _post_inputs(Kc, torch.float32)
    eye = torch.eye(Kc).expand(3, Kc, Kc).contiguous().to(dev)
    for name in ("a NaN entry (tail)", "both infinities in one row", "a row with a negative sum"):
        a = inputs[name]
        for flags in ((True, True, True, True), (False, True, False, False)):
            got = K_.dense_pool(eye, a.to(dev), None, K_.dense_flags(*flags), want_raw=True)
            ref_raw = O.dense_connect(torch.eye(Kc).expand(3, Kc, Kc), a)
            _same(got[1], ref_raw, f"{name} {flags}: raw")
            _same(got[2], O.postprocess_dense(ref_raw, *flags), f"{name} {flags}: adj_pool")


# ================================================================================================ fused losses
def _loss_plants(s0, a0):
    """(what, s, a): one NaN in S; one +inf in A (mirrored: A stays symmetric); an S row of exact zeros and a single 1."""
    s = s0.clone()
    s[0, min(63, s.size(1) - 1), 1] = NAN
    yield "a NaN in S", s, a0
    a = a0.clone()
    a[0, 2, 5] = a[0, 5, 2] = INF
    yield "+inf in A", s0, a
    s = s0.clone()
    s[0, 3] = 0.0
    s[0, 3, 2] = 1.0
    yield "a one-hot row of S", s, a0


def _loss_refs(s, a, n_nodes):
    raw = O.dense_connect(s, a)
    return dict(link=O.link_pred_loss(s, a, False), entropy=O.entropy_loss(s, n_nodes),
                cut=O.mincut_loss(a, s, raw), ortho=O.orthogonality_loss(s))


def _loss_problem(B, N, K, seed):
    g = _gen(seed)
    s = torch.softmax(torch.randn(B, N, K, generator=g), -1)
    up = torch.triu((torch.rand(B, N, N, generator=g) < 0.3).float() * _vals((B, N, N), g), 1)
    return s, up + up.transpose(1, 2)


@pytest.mark.parametrize("shape", [(3, 70, 6), (64, 40, 12)], ids=["B3-N70", "B64-N40"])
def test_dense_losses_every_route_agrees_with_the_oracle(dev, shape):
    """The four dense losses (utils/losses.py) through every route that produces them: the composed functions of
    ``tgp.utils.losses``; ``diffpool_loss_tail`` and ``mincut_loss_terms`` (the one-launch tails); for the batch of
    small graphs the per-graph records of the pooling kernel with ``diffpool_stats_tail_kernel`` and the MinCut tails
    taken inside it.  Each loss is NaN, or infinite with the oracle's sign, exactly where the oracle's is."""
    from tgp import kernels as K
    from tgp.utils import losses as L
    B, N, Kc = shape
    s0, a0 = _loss_problem(B, N, Kc, 61)
    x = _vals((B, N, 4), _gen(62), signed=True)
    small = K.dense_pool_is_small(B, N, Kc, 4)
    assert small == (B == 64)
    flags = K.dense_flags(True, True, True, False)
    assert _all_finite(*_loss_refs(s0, a0, B * N).values())
    cases = _Cases()
    for what, s, a in [("clean", s0, a0)] + list(_loss_plants(s0, a0)):
        ref = _loss_refs(s, a, B * N)
        sd, ad = s.to(dev), a.to(dev)
        raw = K.dense_pool(sd, ad, None, 0, want_raw=True)[1]
        got = {"composed": dict(link=L.link_pred_loss(sd, ad, False), entropy=L.entropy_loss(sd, B * N),
                                cut=L.mincut_loss(ad, sd, raw), ortho=L.orthogonality_loss(sd))}
        both = K.diffpool_loss_tail(sd, ad, None, 1.0, 1.0 / (B * N))
        terms = L.mincut_loss_terms(ad, sd, raw).mean(dim=1)
        got["tails"] = dict(link=both[0], entropy=both[1], cut=terms[0], ortho=terms[1])
        if small:
            out = K.dense_pool(sd, ad, x.to(dev), flags, want_raw=True, diff_stats=True)
            assert out[3] is not None, "the one-wave-per-graph kernel did not take the batch"
            rec = K.diffpool_stats_tail(out[3], 1.0, 1.0 / (B * N))
            out = K.dense_pool(sd, ad, x.to(dev), flags, want_raw=True, mincut_terms=True)
            assert out[3] is not None
            t = out[3].mean(dim=1)
            got["records"] = dict(link=rec[0], entropy=rec[1], cut=t[0], ortho=t[1])
        for route, vals in got.items():
            for name, v in vals.items():
                cases.same(v.reshape(()), ref[name], f"{shape} {what}: {name} on the {route} route")
    cases.done()


@pytest.mark.parametrize("batched", [True, False], ids=["graphs", "single"])
def test_unbatched_losses_and_their_tail(dev, batched):
    """The sparse / unbatched forms (``sparse_mincut_loss``, ``unbatched_orthogonality_loss``, ``sparse_link_pred_loss``,
    ``unbatched_entropy_loss``) and the tail the unbatched and the rows route of DiffPool end in
    (``diffpool_unbatched_tail``: ``diffpool_u_final_kernel``), fed with the products the route forms."""
    from tgp import kernels as K
    from tgp.utils import losses as L
    g = _gen(63)
    sizes = [70, 33] if batched else [103]
    n, Kc = sum(sizes), 6
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    key = torch.unique(torch.randint(0, n * n, (500,), generator=g))
    ei = torch.stack([key // n, key % n])
    ei = ei[:, batch[ei[0]] == batch[ei[1]]]
    w0 = _vals((ei.size(1),), g)
    s0 = torch.softmax(torch.randn(n, Kc, generator=g), -1)
    b_arg = batch if batched else None

    def refs(s, w):
        return dict(cut=O.sparse_mincut_loss(ei, s, w, b_arg), ortho=O.unbatched_orthogonality_loss(s, b_arg),
                    link=O.sparse_link_pred_loss(s, ei, w, b_arg, False), entropy=O.entropy_loss(s, n))
    assert _all_finite(*refs(s0, w0).values())
    s1 = s0.clone()
    s1[63, 1] = NAN
    w1 = w0.clone()
    w1[ei.size(1) - 2] = INF
    s2 = s0.clone()
    s2[3] = 0.0
    s2[3, 2] = 1.0
    cases = _Cases()
    for what, s, w in (("clean", s0, w0), ("a NaN in S", s1, w0), ("+inf in A", s0, w1), ("a one-hot row of S", s2, w0)):
        ref = refs(s, w)
        sd, eid, wd = s.to(dev), ei.to(dev), w.to(dev)
        bd = None if b_arg is None else batch.to(dev)
        got = dict(cut=L.sparse_mincut_loss(eid, sd, wd, bd), ortho=L.unbatched_orthogonality_loss(sd, bd),
                   link=L.sparse_link_pred_loss(sd, eid, wd, bd, False), entropy=L.unbatched_entropy_loss(sd, n))
        for name, v in got.items():
            cases.same(v.reshape(()), ref[name], f"{what}: {name} (composed)")
        # the tail of the unbatched / rows route: raw_b = S_b^T A_b S_b and G_b = S_b^T S_b per graph, sum of w^2
        raw = O.dense_connect_unbatched(ei, w, b_arg, s).to(dev)
        parts = s.split(sizes)
        gram = torch.stack([p.t() @ p for p in parts]).to(dev)
        both = K.diffpool_unbatched_tail(raw, gram, sd, torch.dot(wd, wd), 1.0, 1.0 / n)
        cases.same(both[0].reshape(()), ref["link"], f"{what}: link loss (diffpool_u_final_kernel)")
        cases.same(both[1].reshape(()), ref["entropy"], f"{what}: entropy loss (diffpool_u_final_kernel)")
    cases.done()


POOLER_INPUTS = {  # the dense poolers end to end; `via`: the tgp.kernels call that tells which route an input took
    "small graphs, records + stats tail": dict(sizes=[40] * 64, k=5, alias="diff", via="diffpool_stats_tail"),
    "un-padded rows route": dict(sizes=[300, 257], k=5, alias="diff", via="pool_rows_forward"),
    "unbatched pooler": dict(sizes=[70, 33], k=5, alias="diff_u", via="pool_rows_forward"),
}


@pytest.mark.parametrize("name", sorted(POOLER_INPUTS))
def test_diffpool_losses_through_the_poolers(dev, monkeypatch, name):
    """``get_pooler("diff")`` / ``("diff_u")`` with a NaN feature (its row of S is NaN) and with an infinite edge
    weight: losses, pooled features and pooled adjacency against ``O.dense_pool`` on the routes the input regimes take
    (the records of the one-wave-per-graph kernel with ``diffpool_stats_tail``; the one-call forward of the un-padded
    rows, which ends in ``diffpool_u_final_kernel``, for the batched pooler on large sparse graphs and for ``diff_u``)."""
    from tgp import kernels as K
    from tgp.poolers import get_pooler
    cfg = POOLER_INPUTS[name]
    g = _gen(64)
    sizes, k, f = cfg["sizes"], cfg["k"], 6
    n = sum(sizes)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    start = torch.cumsum(torch.tensor(sizes), 0) - torch.tensor(sizes)
    src = torch.arange(n).repeat_interleave(2)
    dst = start[batch[src]] + (torch.rand(src.numel(), generator=g) * torch.tensor(sizes)[batch[src]]).long()
    key = torch.unique(torch.cat([src * n + dst, dst * n + src]))
    ei = torch.stack([key // n, key % n])
    ei = ei[:, ei[0] != ei[1]]
    w0 = _vals((ei.size(1),), g)
    x0 = _vals((n, f), g, signed=True)
    torch.manual_seed(5)
    pooler = get_pooler(cfg["alias"], in_channels=f, k=k).to(dev).eval()
    lin = pooler.selector.mlp.lins[0]
    wb = [lin.weight.detach().cpu()], [lin.bias.detach().cpu()]
    calls = []
    real = getattr(K, cfg["via"])

    def counted(*a_, **k_):
        out = real(*a_, **k_)
        calls.append(out is not None)
        return out
    monkeypatch.setattr(K, cfg["via"], counted)
    x1 = x0.clone()
    x1[sizes[0] - 1, 2] = NAN
    w1 = w0.clone()
    w1[3] = INF
    cases = _Cases()
    for what, x, w in (("clean", x0, w0), ("a NaN feature", x1, w0), ("an infinite edge weight", x0, w1)):
        calls.clear()
        with torch.no_grad():
            out = pooler(x=x.to(dev), adj=ei.to(dev), edge_weight=w.to(dev), batch=batch.to(dev))
        assert calls and all(calls), f"{name}: {cfg['via']} did not take the call ({calls})"
        ref = O.dense_pool(cfg["alias"].split("_")[0], x, ei, w, batch, *wb, batched=not cfg["alias"].endswith("_u"))
        if what == "clean":
            assert _all_finite(ref["x"], ref["edge_index"], *ref["loss"].values())
        for lname, val in ref["loss"].items():
            cases.same(out.loss[lname].reshape(()), val, f"{name}, {what}: {lname}")
        cases.same(out.x.reshape(ref["x"].shape), ref["x"], f"{name}, {what}: x")
        cases.same(out.edge_index, ref["edge_index"], f"{name}, {what}: adj_pool")
    cases.done()


# ======================================================================================================== TopK
SCORES = [0.5, INF, -1.0, NAN, -INF, 0.5, 2.0, -0.0, 0.0]


def _topk_batch(sizes, seed, shuffle_batch=False):
    """The nine scores tiled to sum(sizes) and shuffled; ties everywhere (the stable order decides: lower node first)."""
    g = _gen(seed)
    n = sum(sizes)
    score = torch.tensor(SCORES).repeat(n // 9 + 1)[:n][torch.randperm(n, generator=g)]
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    if shuffle_batch:
        batch = batch[torch.randperm(n, generator=g)]
    return score, batch


TOPK_SHAPES = {  # sizes, unsorted batch, the sort the selector takes
    "one wave per graph": ([9, 64, 1, 37], False),
    "one workgroup per graph": ([9, 700, 2048, 65], False),
    "beyond the workgroup sort": ([2049, 100], False),
    "device-wide radix (unsorted batch)": ([700, 65, 9], True),
}


@pytest.mark.parametrize("mode", [0.5, 3, 700], ids=["ratio0.5", "ratio3", "ratio700"])
@pytest.mark.parametrize("shape", sorted(TOPK_SHAPES))
def test_topk_ratio_mode(dev, shape, mode):
    """``TopkSelect`` in ratio mode (a fraction and an integer) over the score vector with NaN, both infinities, ties and
    both zeros: ``node_index`` and ``cluster_index`` bit for bit, the weights with the same non-finite positions."""
    from tgp.select import TopkSelect
    from tgp.utils.ops import batch_info
    sizes, unsorted = TOPK_SHAPES[shape]
    score, batch = _topk_batch(sizes, 71, unsorted)
    bd = batch.to(dev)
    info = batch_info(bd)
    assert info.is_sorted == (not unsorted)
    if not unsorted:  # the facts the selector picks its sort by
        lim = {"one wave per graph": (1, 64), "one workgroup per graph": (65, 2048), "beyond the workgroup sort": (2049, 1 << 30)}
        lo, hi = lim[shape]
        assert lo <= info.max_nodes <= hi
    so = TopkSelect(in_channels=None, ratio=mode, act="linear").to(dev)(score.view(-1, 1).to(dev), batch=bd)
    ni, ci, w = O.topk_select(score, None, mode, batch, act="linear")
    assert so.num_supernodes == ni.numel()
    assert torch.equal(so.node_index.cpu(), ni) and torch.equal(so.cluster_index.cpu(), ci)
    _same(so.weight, w, f"{shape} ratio={mode}: weights")
    assert bool(torch.isnan(w).any())  # NaN sorts first, then +inf: kept
    assert mode == 3 or bool(torch.isinf(w).any())


@pytest.mark.parametrize("shape", ["one wave per graph", "one workgroup per graph", "beyond the workgroup sort"])
def test_topk_min_score_mode(dev, shape):
    """``min_score`` mode (per-graph softmax, csrc/topk_select.hip topk_minscore_kernel): a graph that holds a NaN or
    +inf has NaN probabilities and keeps no node; a graph of finite scores keeps what the oracle keeps."""
    from tgp.select import TopkSelect
    sizes, _ = TOPK_SHAPES[shape]
    score, batch = _topk_batch(sizes, 72)
    finite = _vals((sizes[-1],), _gen(73), signed=True)   # the last graph: finite scores, -inf among them
    finite[1] = -INF
    score[-sizes[-1]:] = finite
    for min_score in (0.2, 0.001):
        so = TopkSelect(in_channels=None, min_score=min_score, act="linear").to(dev)(score.view(-1, 1).to(dev),
                                                                                      batch=batch.to(dev))
        ni, ci, w = O.topk_select(score, None, 0.5, batch, min_score=min_score, act="linear")
        assert bool((batch[ni] == len(sizes) - 1).any())  # the finite graph keeps nodes
        poisoned = torch.unique(batch[torch.isnan(score) | (score == INF)])
        assert poisoned.numel() > 0 and not bool(torch.isin(batch[ni], poisoned).any())  # a NaN / +inf graph keeps none
        assert torch.equal(so.node_index.cpu(), ni) and torch.equal(so.cluster_index.cpu(), ci)
        _same(so.weight, w, f"{shape} min_score={min_score}: weights")


def test_topk_entry_points(dev):
    """``tgp.kernels.topk_minscore`` and ``tgp.kernels.topk_select`` called directly."""
    from tgp import kernels as K
    sizes = [9, 700, 65]
    score, batch = _topk_batch(sizes, 74)
    ptr = torch.tensor([0, 9, 709, 774])
    score[9:709] = _vals((700,), _gen(75), signed=True)  # one finite graph
    prob, node_index = K.topk_minscore(score.to(dev), ptr.to(dev), 0.002)
    nb = 3
    smax = O.seg_reduce(score, batch, nb, "max")
    e = (score - smax[batch]).exp()
    want = e / (O.seg_sum(e, batch, nb) + 1e-16)[batch]
    _same(prob, want, "topk_minscore: probabilities")
    assert torch.equal(node_index.cpu(), O.topk_perm(want, 0.5, batch, min_score=0.002))
    k, koff = K.topk_plan(torch.tensor(sizes).to(dev), 0.5)
    index, assign, values = K.topk_select(score.to(dev), batch.to(dev), nb, ptr.to(dev), k, koff, int(koff[-1]),
                                          segments_max_nodes=700, with_values=True)
    ni, ci, w = O.topk_select(score, None, 0.5, batch, act="linear")
    assert torch.equal(index[0].cpu(), ni) and torch.equal(index[1].cpu(), ci)
    _same(values, w, "topk_select: values")


@pytest.mark.parametrize("sizes", [[9, 64, 37], [700, 65]], ids=["small graphs", "large graphs"])
def test_topk_pooler_end_to_end(dev, sizes):
    """``get_pooler("topk")``: the kept NaN / infinite score multiplies its row of x, so the pooled features carry
    the same non-finite positions; node_index, cluster_index, the pooled batch and edge_index are equal."""
    from tgp.poolers import get_pooler
    g = _gen(76)
    f = 8
    score, batch = _topk_batch(sizes, 77)
    n = score.numel()
    x = _vals((n, f), g, signed=True)
    x[:, 0] = score
    ei = torch.stack([torch.sort(torch.randint(0, n, (4 * n,), generator=g))[0], torch.randint(0, n, (4 * n,), generator=g)])
    ei = ei[:, batch[ei[0]] == batch[ei[1]]]
    ew = _vals((ei.size(1),), g)
    pooler = get_pooler("topk", in_channels=f, ratio=0.5, nonlinearity="linear").to(dev).eval()
    p = torch.zeros(1, f)
    p[0, 0] = 1.0  # score = x[:, 0] exactly (the other products are +-0), so CPU and GPU rank the same numbers
    with torch.no_grad():
        pooler.selector.weight.copy_(p)
        out = pooler(x=x.to(dev), adj=ei.to(dev), edge_weight=ew.to(dev), batch=batch.to(dev))
    xz = x.clone()
    xz[~torch.isfinite(xz)] = 1.0
    assert _all_finite(O.topk_pool(xz, ei, ew, batch, p, ratio=0.5, act="linear")["x"])
    ref = O.topk_pool(x, ei, ew, batch, p, ratio=0.5, act="linear")
    assert torch.equal(out.so.node_index.cpu(), ref["node_index"])
    assert torch.equal(out.so.cluster_index.cpu(), ref["cluster_index"])
    assert torch.equal(out.batch.cpu(), ref["batch"]) and torch.equal(out.edge_index.cpu(), ref["edge_index"])
    _same(out.edge_weight, ref["edge_weight"], "topk pooler: edge weights")
    _same(out.x, ref["x"], "topk pooler: pooled x")
    assert bool(torch.isnan(ref["x"]).any()) and bool(torch.isinf(ref["x"]).any())


# =================================================================================================== MLPSelect
@pytest.mark.parametrize("n", [5, 257])
@pytest.mark.parametrize("k", [3, 33])
def test_mlp_select(dev, k, n):
    """``MLPSelect`` (one Linear + softmax, csrc/mlp_select.hip) against ``O.mlp_select``: an infinite feature makes its
    row's logits infinite (the softmax row is NaN), a NaN feature makes its row NaN, and no other row changes; a bias of
    -inf puts one -inf into every row (that column is 0, the rows stay finite); every bias -inf, one bias +inf or one
    bias NaN makes every row NaN."""
    from tgp import kernels as K
    from tgp.select import MLPSelect
    g = _gen(81)
    cases = _Cases()
    for f in (7, 32):
        assert k <= K.N.lib().tgp_mlp_select_max_fused_k()
        sel = MLPSelect(in_channels=f, k=k).to(dev).eval()
        w0, b0 = _vals((k, f), g, signed=True), _vals((k,), g, signed=True)
        x0 = _vals((2, n, f), g, signed=True)
        mask = torch.ones(2, n, dtype=torch.bool)
        mask[1, n - 2:] = False

        def run(x, w, b, what, entry=False):
            with torch.no_grad():
                sel.mlp.lins[0].weight.copy_(w)
                sel.mlp.lins[0].bias.copy_(b)
                got = sel(x.to(dev), mask=mask.to(dev)).s
                if entry:  # the C entry point, called directly
                    direct = K.mlp_select(x.to(dev), w.to(dev), b.to(dev), mask.to(dev))
                    assert torch.equal(direct.isnan(), got.isnan())
                    cases.same(direct, O.mlp_select(x, [w], [b], mask), f"k={k} n={n} F={f} {what} (tgp.kernels)")
            ref = O.mlp_select(x, [w], [b], mask)
            cases.same(got, ref, f"k={k} n={n} F={f} {what}")
            return ref
        assert _all_finite(run(x0, w0, b0, "clean"))
        for kind, where in itertools.product(("nan", "+inf", "-inf"), ("first", "last", "tail", "tile_row")):
            x = x0.clone()
            pos = plant(x[0], kind, where, g, tile=32)
            ref = run(x, w0, b0, f"{kind} feature ({where})", entry=where == "tail")
            bad = torch.isnan(ref[0]).any(-1).nonzero().view(-1)
            assert bad.tolist() == [int(pos[0, 0])] and _all_finite(ref[1])  # its row, whole, and no other
        b = b0.clone()
        b[k - 1] = -INF
        ref = run(x0, w0, b, "one -inf logit per row", entry=True)
        assert _all_finite(ref) and bool((ref[..., k - 1] == 0).all())
        assert bool(torch.isnan(run(x0, w0, torch.full((k,), -INF), "all logits -inf")[mask]).all())
        b = b0.clone()
        b[0] = INF
        assert bool(torch.isnan(run(x0, w0, b, "one +inf logit per row")[mask]).all())
        b = b0.clone()
        b[1] = NAN  # ONE NaN among finite logits: the row maximum skips it, the exponential must not
        assert bool(torch.isnan(run(x0, w0, b, "one NaN logit per row", entry=True)[mask]).all())
    cases.done()


# ===================================================================================================== Graclus
def _graclus_graph(sizes, seed):
    """A sorted batch: per graph random undirected pairs with distinct finite weights, a fifth of them NaN (both
    directions), a few -inf, node-disjoint +inf pairs, and two extra nodes p, q: q's only neighbour is p, and p's other
    entries are NaN-weighted -- so (p, q) must be matched.  Both directions listed, sorted by (row, col)."""
    g = _gen(seed)
    rows, cols, ws, inf_pairs, pendants, off = [], [], [], [], [], 0
    for m in sizes:
        core = m - 2
        a = torch.randint(0, core, (2 * core,), generator=g)
        b = torch.randint(0, core, (2 * core,), generator=g)
        keep = a != b
        lo, hi = torch.minimum(a, b)[keep], torch.maximum(a, b)[keep]
        key = torch.unique(lo * core + hi)
        lo, hi = key // core, key % core
        w = (torch.randperm(key.numel(), generator=g).double() / key.numel() * 1.95 + 0.05).float()  # distinct
        r = torch.rand(key.numel(), generator=g)
        w[r < 0.2] = NAN
        w[(r >= 0.2) & (r < 0.25)] = -INF
        used = set()
        for e in (r >= 0.5).nonzero().view(-1).tolist()[: max(core // 10, 1) * 3]:
            u, v = int(lo[e]), int(hi[e])
            if u not in used and v not in used:
                used.update((u, v))
                w[e] = INF
                inf_pairs.append((off + u, off + v))
        p, q = core, core + 1
        others = torch.randperm(core, generator=g)[:2]
        lo = torch.cat([lo, torch.tensor([p]), others])
        hi = torch.cat([hi, torch.tensor([q]), torch.tensor([p, p])])
        w = torch.cat([w, torch.tensor([0.7, NAN, NAN])])
        pendants.append((off + p, off + q))
        rows += [lo + off, hi + off]
        cols += [hi + off, lo + off]
        ws += [w, w]
        off += m
    row, col, w = torch.cat(rows), torch.cat(cols), torch.cat(ws)
    order = torch.argsort(row * off + col)
    return torch.stack([row[order], col[order]]), w[order], off, inf_pairs, pendants


def _check_matching(cluster, ei, w, n, inf_pairs, pendants, what):
    """``cluster`` [n]: an id per node, equal for the two nodes of a pair."""
    counts = torch.bincount(cluster)
    assert int(counts.max()) <= 2, f"{what}: a cluster of more than two nodes"
    matched = counts[cluster] == 2
    ok = ~torch.isnan(w) & (ei[0] != ei[1])
    joined = cluster[ei[0]] == cluster[ei[1]]
    # every pair is joined by an entry whose weight is not NaN ...
    has_edge = torch.zeros(n, dtype=torch.bool)
    has_edge[ei[0][ok & joined]] = True
    assert bool(has_edge[matched].all()), f"{what}: a pair that no entry with a real weight joins"
    # ... and the matching is maximal over those entries: no such entry between two free nodes
    free = ~matched
    assert not bool((ok & free[ei[0]] & free[ei[1]]).any()), f"{what}: a free node whose free neighbour went unmatched"
    for u, v in inf_pairs:
        assert cluster[u] == cluster[v], f"{what}: the +inf entry ({u}, {v}) lost to a finite one"
    for p, q in pendants:
        assert cluster[p] == cluster[q], f"{what}: node {q}'s only neighbour {p} was free and was not taken"


GRACLUS_SHAPES = {"one wave": [9, 64, 33, 50, 64, 12], "one workgroup": [65, 700, 300], "device-wide": [5000]}


@pytest.mark.parametrize("shape", sorted(GRACLUS_SHAPES))
def test_graclus_contract_with_nan_and_infinite_weights(dev, monkeypatch, shape):
    """Graclus's own rule (csrc/graclus_match.hip: "NaN weights never match"): the matching is valid, no pair is joined
    only by a NaN-weighted entry, it is maximal over the other entries (a node whose only real neighbour is free gets
    matched), +inf beats every finite weight, and two runs give equal bits -- on the one-launch one-wave route, the
    one-workgroup-per-graph route and the device-wide rounds.

    Round bounds, from the loops (none depends on the weights: a round either matches a pair -- the free set loses two
    nodes and never grows -- or matches nothing and ends the loop; a NaN entry is never a candidate, so it can neither
    match nor keep a round alive): gm_graph_fused_kernel at most 64 / 2 + 1 rounds (hard cap 2 * 64 + 2);
    gm_graph_rounds at most n_graph / 2 + 1 <= 513 (hard cap 2 * GM_GRAPH_MAX); gm_tail_rounds_kernel at most
    GM_TAIL_CAP / 2 + 1; the host loop of tgp_graclus_match_rounds at most n / 2 rounds that match plus one batch of at
    most 256 rounds whose last flag is 0; gm_steal_long_rows ends when its ticket counter reaches the list's length."""
    from tgp import kernels as KK
    from tgp.select import GraclusSelect
    sizes = GRACLUS_SHAPES[shape]
    ei, w, n, inf_pairs, pendants = _graclus_graph(sizes, 91)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(sizes).cumsum(0)])
    lib = KK.N.lib()
    calls = {"tgp_graclus_match_graphs_fused": 0, "tgp_graclus_match_graphs": 0, "tgp_graclus_match_rounds": 0}
    for name in calls:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a_, _n=name, _r=real: (calls.__setitem__(_n, calls[_n] + 1), _r(*a_))[1])
    eid, wd = ei.to(dev), w.to(dev)
    runs = []
    for _ in range(2):
        if shape == "one wave":
            assert max(sizes) <= 64
            index, k, _, _ = KK.graclus_match(eid, wd, n, graph_ptr=ptr.to(dev), max_graph_nodes=max(sizes), relabel=True)
            runs.append(index[1].cpu())
        elif shape == "one workgroup":
            assert 64 < max(sizes) <= lib.tgp_graclus_match_max_graph_nodes()
            runs.append(KK.graclus_match(eid, wd, n, graph_ptr=ptr.to(dev), max_graph_nodes=max(sizes)).cpu())
        else:
            runs.append(KK.graclus_match(eid, wd, n).cpu())
    took = {"one wave": "tgp_graclus_match_graphs_fused", "one workgroup": "tgp_graclus_match_graphs",
            "device-wide": "tgp_graclus_match_rounds"}[shape]
    assert calls[took] >= 2 and (shape == "device-wide" or calls["tgp_graclus_match_rounds"] == 0), calls
    assert torch.equal(runs[0], runs[1]), "two runs differ"
    _check_matching(runs[0], ei, w, n, inf_pairs, pendants, shape)
    so = GraclusSelect()(eid, wd, num_nodes=n, batch=batch.to(dev) if shape != "device-wide" else None)
    _check_matching(so.cluster_index.cpu(), ei, w, n, inf_pairs, pendants, shape + " (GraclusSelect)")
    assert so.num_supernodes == int(so.cluster_index.max()) + 1
