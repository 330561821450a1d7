"""NMF pooling on the device: the per-graph coordinate-descent kernel of csrc/nmf.hip, its default init, the status word
and the routes, against the reference's stored results (tests/golden/golden_nmf_v1.pt, pinned through ``init=``) and
against the float64 restatement (tests/nmf_restatement.py)."""
import functools
import os

import pytest
import torch

import nmf_restatement as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BLOB = torch.load(os.path.join(HERE, "golden", "golden_nmf_v1.pt"), weights_only=True)
CASES, OPTS = BLOB["cases"], BLOB["opts"]
TOL = dict(rtol=1e-5, atol=1e-5)
SHAPE_SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 128]  # around k = 2, 3, 32, the 64-node thread-count switch, the limit


def dev():
    return torch.device("cuda:0")


def limits():
    from tgp import kernels as K
    return K.nmf_max_nodes(), K.nmf_max_k()


def random_batch(sizes, seed, degree=5.0):
    """Directed random graphs (about ``degree`` out-edges per node), weights in [0.1, 1): (edge_index, weight, batch)."""
    g = torch.Generator().manual_seed(seed)
    eis, ews, bs, off = [], [], [], 0
    for gi, n in enumerate(sizes):
        a = (torch.rand(n, n, generator=g) < min(0.5, degree / max(n, 1))) * (torch.rand(n, n, generator=g) * 0.9 + 0.1)
        idx = a.nonzero().t()
        eis.append(idx + off)
        ews.append(a[idx[0], idx[1]])
        bs.append(torch.full((n,), gi, dtype=torch.long))
        off += n
    return torch.cat(eis, 1), torch.cat(ews), torch.cat(bs)


def select(ei, ew, batch, k, **kw):
    from tgp.select import nmf_select
    d = dev()
    init = kw.pop("init", None)
    if init is not None:
        init = (init[0].to(d), init[1].to(d))
    return nmf_select(ei.to(d), k, None if ew is None else ew.to(d), None if batch is None else batch.to(d), init=init, **kw)


def check_adj(out, want, tol):
    if "dense" in want:
        assert out.edge_weight is None
        torch.testing.assert_close(out.edge_index.cpu(), want["dense"], **tol)
    else:
        assert torch.equal(out.edge_index.cpu(), want["edge_index"])
        torch.testing.assert_close(out.edge_weight.cpu(), want["edge_weight"], **tol)


# ------------------------------------------------------------------------------------------------ fixture parity
@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_the_reference_through_init(name):
    from tgp.poolers import NMFPooling
    c = CASES[name]
    i, d = c["inputs"], dev()
    n = i["x"].size(0)
    so, fac = select(i["edge_index"], i["edge_weight"], i["batch"], c["k"], num_nodes=n, fixed_k=c["fixed_k"],
                     tol=c["tol"], max_iter=c["max_iter"], init=(c["w0"], c["h0t"]), return_factors=True)
    want = c["expected"]
    assert so.s.dtype == torch.float32 and tuple(so.s.shape) == tuple(want["s"].shape)
    torch.testing.assert_close(so.s.cpu(), want["s"], **TOL)
    torch.testing.assert_close(so.s.cpu().double(), c["f64"]["s"], **TOL)
    assert fac["iters"].cpu().tolist() == c["sklearn_iter"] == c["f64"]["iters"]
    for gi, it in enumerate(c["sklearn_iter"]):  # the stored margins of the stopping test, seen from the kernel's side
        if it > 0:
            assert float(fac["ratio"][gi]) <= c["tol"]
    x = i["x"].to(d)
    for oi, opts in enumerate(OPTS):
        b = i["batch"]
        if b is None and opts["sparse_output"]:
            b = torch.zeros(n, dtype=torch.long)
        pooler = NMFPooling(k=c["k"], **opts)
        so_b = so if b is i["batch"] else type(so)(s=so.s, s_inv_op="transpose", batch=b.to(d))
        out = pooler(x=x, adj=i["edge_index"].to(d), edge_weight=i["edge_weight"].to(d), so=so_b,
                     batch=None if b is None else b.to(d))
        check_adj(out, want["adj"][oi], TOL)
        if oi == 0:
            torch.testing.assert_close(out.x.cpu().reshape(want["x_pool"].shape), want["x_pool"], **TOL)
            lift = pooler(x=out.x, so=so, batch=None if b is None else b.to(d), batch_pooled=out.batch, lifting=True)
            torch.testing.assert_close(lift.cpu(), want["lift"], **TOL)


# ------------------------------------------------------------------------------------------------ fixed iteration counts
@functools.lru_cache(maxsize=None)
def fixed_iteration_problem():
    sizes = [5, 17, 40, 64, 65, 96, 128]
    ei, ew, batch = random_batch(sizes, 11)
    return sizes, ei, ew, batch


@functools.lru_cache(maxsize=None)
def fixed_iteration_reference(k, T):
    sizes, ei, ew, batch = fixed_iteration_problem()
    f64 = R.nmf_select(ei, k, ew, batch, seed=3, tol=0.0, max_iter=T, dtype=torch.float64)
    # (ordered: sums written out one addition at a time, so the yardstick does not depend on the host's BLAS or threads)
    f32 = R.nmf_select(ei, k, ew, batch, seed=3, tol=0.0, max_iter=T, dtype=torch.float32, ordered=True)
    return f64, f32


@pytest.mark.parametrize("T", [1, 3, 10])
@pytest.mark.parametrize("k", [4, 32])
def test_fixed_iteration_counts_against_float64(k, T):
    """Raw W and H^T after exactly T iterations.  The bound per graph is 4 x the error of the fp32 CPU restatement against
    the float64 one on the same input (the reference arithmetic's own error; the margin covers a different but fixed
    summation order) plus a 1e-6 floor -- never anything measured on the kernel.  The float64 run starts from the float64
    default init, whose ``avg`` the fp32 runs round: that rounding is inside the fp32 restatement's error too.
    The fp32 restatement adds every sum one rounded term at a time (``ordered=True``), so the yardstick is the same
    number on every host, whatever its BLAS and thread count.  Measured (profiles/nmf_forward.txt): the ratio kernel
    error / fp32 restatement error lies in 0.1 .. 1.63 over the 84 comparisons."""
    sizes, ei, ew, batch = fixed_iteration_problem()
    f64, f32 = fixed_iteration_reference(k, T)
    so, fac = select(ei, ew, batch, k, seed=3, tol=0.0, max_iter=T, return_factors=True)
    lo = 0
    for gi, m in enumerate(sizes):
        hi = lo + m
        factorised = 1 < k < m
        assert int(fac["iters"][gi]) == (T if factorised else 0)
        for name in ("w", "ht"):
            ref = f64[name][lo:hi]
            own = float((f32[name][lo:hi].double() - ref).abs().max())
            err = float((fac[name][lo:hi].cpu().double() - ref).abs().max())
            bound = 4.0 * own + 1e-6
            print(f"nmf fixed-iteration k={k} T={T} n={m} {name}: kernel err {err:.3e}, fp32 restatement err {own:.3e}, "
                  f"ratio {err / max(own, 1e-30):.2f}, bound {bound:.3e}")
            assert err <= bound, (gi, name, err, bound)
        lo = hi


# ------------------------------------------------------------------------------------------------ shapes
@functools.lru_cache(maxsize=None)
def shape_problem():
    return random_batch(SHAPE_SIZES, 23)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 32])
def test_shapes_that_can_go_wrong(k):
    """n in {1, 2, 3, 63, 64, 65, max_n} and K in {1, 2, 3, max_k} with K = n - 1, n, n + 1 among them (n = 3 against
    K = 2, 3, 4; n = 31, 32, 33 against K = 32), five iterations from the default init."""
    max_n, max_k = limits()
    assert max(SHAPE_SIZES) == max_n and max_k == 32
    ei, ew, batch = shape_problem()
    ref = R.nmf_select(ei, k, ew, batch, seed=1, tol=0.0, max_iter=5, dtype=torch.float64)
    so, fac = select(ei, ew, batch, k, seed=1, tol=0.0, max_iter=5, return_factors=True)
    assert tuple(so.s.shape) == (sum(SHAPE_SIZES), k)
    torch.testing.assert_close(so.s.cpu().double(), ref["s"], **TOL)
    assert fac["iters"].cpu().tolist() == ref["iters"]
    assert [it > 0 for it in ref["iters"]] == [1 < k < m for m in SHAPE_SIZES]


def test_all_special_cases_in_one_batch_and_empty_inputs():
    from tgp.select import nmf_select
    d = dev()
    # no nodes (graph 1, in the middle), ones (n = 1), identity (n = 3 <= k), factorised (n = 9), no edges (n = 6)
    sizes = [1, 0, 3, 9, 6]
    ei, ew, b = random_batch([1, 3, 9], 5)
    batch = torch.tensor([0] + [2] * 3 + [3] * 9 + [4] * 6)
    ref = R.nmf_select(ei, 4, ew, batch, num_nodes=19, dtype=torch.float64)
    so, fac = select(ei, ew, batch, 4, return_factors=True)
    torch.testing.assert_close(so.s.cpu().double(), ref["s"], **TOL)
    assert fac["iters"].cpu().tolist() == ref["iters"] and ref["iters"][4] == 1 and ref["iters"][1] == 0
    s = so.s.cpu()
    assert torch.equal(s[0], torch.tensor([1.0, 0, 0, 0])) and torch.equal(s[1:4, :3], torch.eye(3))
    assert torch.equal(s[13:], torch.full((6, 4), 0.25))  # the all-zero adjacency: uniform after one iteration
    # E = 0 for the whole batch, and no nodes at all
    so = select(torch.zeros(2, 0, dtype=torch.long), None, torch.tensor([0] * 5 + [1] * 2), 3)
    assert torch.equal(so.s.cpu(), torch.cat([torch.full((5, 3), 1 / 3), torch.tensor([[1.0, 0, 0], [0, 1.0, 0]])]))
    so = nmf_select(torch.zeros(2, 0, dtype=torch.long, device=d), 3, batch=torch.zeros(0, dtype=torch.long, device=d))
    assert tuple(so.s.shape) == (0, 0)
    so = nmf_select(torch.zeros(2, 0, dtype=torch.long, device=d), 3, fixed_k=True)
    assert tuple(so.s.shape) == (0, 3)


# ------------------------------------------------------------------------------------------------ routing
def test_composed_routes_agree_with_the_restatement():
    max_n, max_k = limits()
    # a graph past the node limit between two that are not: rows in node order, the middle one composed
    sizes = [20, max_n + 1, 30]
    ei, ew, batch = random_batch(sizes, 31)
    ref = R.nmf_select(ei, 4, ew, batch, seed=2, tol=0.0, max_iter=3, dtype=torch.float64)
    so, fac = select(ei, ew, batch, 4, seed=2, tol=0.0, max_iter=3, return_factors=True)
    torch.testing.assert_close(so.s.cpu().double(), ref["s"], **TOL)
    torch.testing.assert_close(fac["ht"].cpu().double(), ref["ht"], **TOL)
    assert fac["iters"].cpu().tolist() == [3, 3, 3]
    # K past its limit: every graph composed (the identity for n <= K)
    ei, ew, batch = random_batch([12, 40], 32)
    ref = R.nmf_select(ei, max_k + 1, ew, batch, seed=2, tol=0.0, max_iter=2, dtype=torch.float64)
    so, fac = select(ei, ew, batch, max_k + 1, seed=2, tol=0.0, max_iter=2, return_factors=True)
    torch.testing.assert_close(so.s.cpu().double(), ref["s"], **TOL)
    assert fac["iters"].cpu().tolist() == [0, 2]
    # float64 weights: float64 out, composed
    ei, ew, batch = random_batch([9, 14], 33)
    ref = R.nmf_select(ei, 3, ew.double(), batch, seed=2, tol=0.0, max_iter=4, dtype=torch.float64)
    so = select(ei, ew.double(), batch, 3, seed=2, tol=0.0, max_iter=4)
    assert so.s.dtype == torch.float64
    torch.testing.assert_close(so.s.cpu(), ref["s"], rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------------------------------------ default init
def test_default_init_matches_the_restatement_and_ignores_the_position():
    from tgp import kernels as K
    d = dev()
    sizes = [7, 40, 7, 23]
    ei, ew, batch = random_batch(sizes, 41)
    # graph 2 := a copy of graph 0
    e0 = (batch[ei[0]] == 0)
    keep = batch[ei[0]] != 2
    ei = torch.cat([ei[:, keep], ei[:, e0] + 47], 1)
    ew = torch.cat([ew[keep], ew[e0]])
    order = torch.sort(batch[ei[0]], stable=True)[1]
    ei, ew = ei[:, order], ew[order]
    k = 3
    by_src = K.edge_group(ei.to(d), batch.numel())
    graphs = K.build_assign_index(batch.to(d), len(sizes))
    w0, h0t, st = K.nmf_init(by_src, ei[1].to(d), ew.to(d), batch.to(d).to(torch.int32), graphs, k, max(sizes), seed=9)
    assert st == 0
    lo = 0
    for m in sizes:
        a = R.dense_adjacency(ei, ew, lo, lo + m).clamp(min=0)
        rw, rh = R.default_init(a, k, 9)
        # avg = sqrt(sum / n^2 / ka): the two sums differ in order, each within (terms - 1) eps of the exact one for
        # non-negative terms -- the kernel adds n row sums of n terms, 2 n eps -- halved by the square root, plus the
        # roundings of the division, the root and the product
        rtol = (2 * m + 4) * 2.0 ** -24
        torch.testing.assert_close(w0[lo:lo + m].cpu(), rw, rtol=rtol, atol=0.0)
        torch.testing.assert_close(h0t[lo:lo + m].cpu(), rh, rtol=rtol, atol=0.0)
        avg = float(torch.sqrt(a.mean() / k))
        assert float(rw.min()) > 0.0 and float(rw.max()) <= 2.0 * avg and float(rh.max()) <= 2.0 * avg
        lo += m
    assert torch.equal(w0[0:7], w0[47:54]) and torch.equal(h0t[0:7], h0t[47:54])
    # the whole selection: the same graph at two positions, a permuted batch, two calls, two seeds
    a = select(ei, ew, batch, k, seed=9).s
    assert torch.equal(a[0:7], a[47:54])
    assert torch.equal(a, select(ei, ew, batch, k, seed=9).s)
    assert not torch.equal(a, select(ei, ew, batch, k, seed=10).s)
    perm_sizes = [sizes[3], sizes[1], sizes[0]]
    starts = {0: 0, 1: 7, 2: 47, 3: 54}
    parts_e, parts_w, off = [], [], 0
    for g in (3, 1, 0):
        sel = batch[ei[0]] == g
        parts_e.append(ei[:, sel] - starts[g] + off)
        parts_w.append(ew[sel])
        off += sizes[g]
    pb = torch.cat([torch.full((m,), j, dtype=torch.long) for j, m in enumerate(perm_sizes)])
    p = select(torch.cat(parts_e, 1), torch.cat(parts_w), pb, k, seed=9).s
    assert torch.equal(p, torch.cat([a[54:77], a[7:47], a[0:7]]))


# ------------------------------------------------------------------------------------------------ status
def raw_factorize(ei, ew, batch, num_graphs, k, sentinel=-7.0):
    """The C entry on hand-made inputs: (status, s) with ``s`` pre-filled with ``sentinel``."""
    from tgp import _native as N
    from tgp import kernels as K
    d = dev()
    n, E = batch.numel(), ei.size(1)
    ei, ew, batch = ei.to(d), ew.to(d).float().contiguous(), batch.to(d)
    by_src = K.edge_group(ei, n)
    graphs = K.build_assign_index(batch, num_graphs)
    gid = batch.to(torch.int32)
    dst = ei[1].contiguous()
    s = torch.full((n, k), sentinel, device=d)
    status = torch.zeros(1, dtype=torch.int32, device=d)
    rc = N.lib().tgp_nmf_factorize_f32(N.ptr(by_src.row_ptr), N.ptr(by_src.perm), N.ptr(dst), N.ptr(ew), N.ptr(gid),
                                       N.ptr(graphs.row_ptr), N.ptr(graphs.perm), n, E, num_graphs, k, k, 16, 0, 1e-4, 50,
                                       None, None, N.ptr(s), None, None, None, None, N.ptr(status), N.stream_ptr(d))
    assert rc == 0
    torch.cuda.synchronize()
    return int(status.item()), s.cpu()


def test_refused_inputs_raise_and_leave_the_flagged_graph_unwritten():
    from tgp import kernels as K
    ei, ew, batch = random_batch([8, 10, 9], 51)
    n = batch.numel()
    at = int((batch[ei[0]] == 1).nonzero()[0])  # an edge of the middle graph
    clean_status, clean = raw_factorize(ei, ew, batch, 3, 3)
    assert clean_status == 0 and bool((clean >= 0).all())
    # an endpoint >= N (a destination: the by-source index is built over the sources)
    bad = ei.clone()
    bad[1, at] = n + 5
    st, s = raw_factorize(bad, ew, batch, 3, 3)
    assert st == K.NMF_BAD_INPUT and bool((s[8:18] == -7.0).all())
    assert torch.equal(s[:8], clean[:8]) and torch.equal(s[18:], clean[18:])
    with pytest.raises(ValueError):
        select(bad, ew, batch, 3)
    # an edge across two graphs
    bad = ei.clone()
    bad[1, at] = 0
    st, s = raw_factorize(bad, ew, batch, 3, 3)
    assert st == K.NMF_BAD_INPUT and bool((s[8:18] == -7.0).all()) and torch.equal(s[:8], clean[:8])
    with pytest.raises(ValueError, match="two graphs"):
        select(bad, ew, batch, 3)
    # a NaN weight
    badw = ew.clone()
    badw[at] = float("nan")
    st, s = raw_factorize(ei, badw, batch, 3, 3)
    assert st == K.NMF_NON_FINITE and bool((s[8:18] == -7.0).all()) and torch.equal(s[18:], clean[18:])
    with pytest.raises(ValueError, match="NaN or infinity"):
        select(ei, badw, batch, 3)
    # a graph past max_n of the launch (16 here): flagged, unwritten, the others done
    ei2, ew2, batch2 = random_batch([8, 17], 52)
    st, s = raw_factorize(ei2, ew2, batch2, 2, 3)
    assert st == K.NMF_OVER_LIMIT and bool((s[8:] == -7.0).all()) and bool((s[:8] >= 0).all())


# ------------------------------------------------------------------------------------------------ memory
def test_a_warm_call_stays_below_one_padded_adjacency():
    sizes = [60] * 64
    ei, ew, batch = random_batch(sizes, 61)
    d = dev()
    ei, ew, batch = ei.to(d), ew.to(d), batch.to(d)
    from tgp.select import nmf_select
    nmf_select(ei, 8, ew, batch, tol=0.0, max_iter=2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    so = nmf_select(ei, 8, ew, batch, tol=0.0, max_iter=2)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"nmf warm call on 64 x 60 nodes: peak rise {rise} bytes against {64 * 60 * 60 * 4} of a padded adjacency")
    assert tuple(so.s.shape) == (3840, 8) and rise < 64 * 60 * 60 * 4


# ------------------------------------------------------------------------------------------------ pooler level
def test_pooler_forward_cache_precoarsening_and_lift():
    from tgp.poolers import NMFPooling
    d = dev()
    sizes = [12, 3, 20]
    ei, ew, batch = random_batch(sizes, 71)
    ei, ew, batch = ei.to(d), ew.to(d), batch.to(d)
    x = torch.randn(35, 6, device=d)
    dense = NMFPooling(k=4, cached=True)
    out = dense(x=x, adj=ei, edge_weight=ew, batch=batch)
    assert tuple(out.x.shape) == (3, 4, 6) and tuple(out.edge_index.shape) == (3, 4, 4) and out.edge_weight is None
    assert tuple(out.so.s.shape) == (35, 4) and torch.equal(out.so.s[12:15, :3], torch.eye(3, device=d))
    torch.testing.assert_close(out.so.s.sum(-1), torch.ones(35, device=d), **TOL)
    again = dense(x=x, adj=ei, edge_weight=ew, batch=batch)
    assert again.so is out.so  # cached
    s3 = torch.zeros(3, 20, 4, device=d)
    pos = torch.cat([torch.arange(m) for m in sizes]).to(d)
    s3[batch, pos] = out.so.s
    x3 = torch.zeros(3, 20, 6, device=d)
    x3[batch, pos] = x
    torch.testing.assert_close(out.x, s3.transpose(1, 2) @ x3, **TOL)
    lifted = dense(x=out.x, so=out.so, batch=batch, batch_pooled=out.batch, lifting=True)
    torch.testing.assert_close(lifted, (s3 @ out.x)[batch, pos], **TOL)
    sparse = NMFPooling(k=4, sparse_output=True)
    out2 = sparse(x=x, adj=ei, edge_weight=ew, so=out.so, batch=batch)
    assert tuple(out2.x.shape) == (12, 6) and out2.edge_index.size(0) == 2 and out2.edge_weight.numel() == out2.edge_index.size(1)
    assert out2.batch.tolist() == [0] * 4 + [1] * 4 + [2] * 4
    torch.testing.assert_close(out2.x, out.x.reshape(12, 6), **TOL)
    # precoarsening of one graph with n < K keeps the width K
    g_ei = ei[:, batch[ei[0]] == 1] - 12
    pre = NMFPooling(k=4).precoarsening(edge_index=g_ei, edge_weight=ew[batch[ei[0]] == 1], num_nodes=3)
    assert tuple(pre.so.s.shape) == (3, 4) and torch.equal(pre.so.s[:, :3], torch.eye(3, device=d))
    assert bool((pre.so.s[:, 3] == 0).all())
