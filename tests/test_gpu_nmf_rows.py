"""The row-walking NMF kernel of csrc/nmf_rows.hip (graphs past the 128-node LDS kernel, no dense adjacency) against the
float64 restatement (tests/nmf_restatement.py): fixed iteration counts, the stopping rule, the routes of one batch, the
declined and refused lists, and the memory of a warm call."""
import functools

import pytest
import torch

import nmf_restatement as R
from test_gpu_nmf import TOL, dev, random_batch, select

pytestmark = pytest.mark.gpu


def rows_direct(ei, ew, batch, k, home="auto", sentinel=0.0, **kw):
    """``kernels.nmf_rows_factorize`` over every graph of the batch, ``s`` pre-filled with ``sentinel``."""
    from tgp import kernels as K
    d = dev()
    n, G = batch.numel(), int(batch.max()) + 1
    ei, ew, batch = ei.to(d), ew.to(d), batch.to(d)
    graphs = K.build_assign_index(batch, G)
    return K.nmf_rows_factorize(K.sag_edge_group(ei, n, by_destination=False), K.sag_edge_group(ei, n, by_destination=True),
                                ei[0], ei[1], ew, batch.to(torch.int32), graphs,
                                torch.arange(G, dtype=torch.int32, device=d), k, k, home=home,
                                s=torch.full((n, k), sentinel, device=d), **kw)


# ------------------------------------------------------------------------------------------------ fixed iteration counts
@functools.lru_cache(maxsize=None)
def fixed_problem(name, k):
    """small: 129 (the first graph past the LDS kernel), 130, 257 (odd: a tail of the 2-deep MFMA step, uneven wave
    slices), a graph with negative weights, a 200-node star (one row and one column of 199 entries), 150 nodes without
    edges.  large: 1024 / 1025 (the second row of a thread) and, for k = 32, the edge of the LDS frame."""
    from tgp import kernels as K
    if name == "large":
        edge = K.nmf_rows_lds_nodes(32)
        sizes = [1024, 1025] + ([edge, edge + 1] if k == 32 else [])
        return (sizes,) + random_batch(sizes, 13)
    sizes = [129, 130, 257, 140]
    ei, ew, batch = random_batch(sizes, 12)
    neg = (batch[ei[0]] == 3).nonzero().view(-1)[::3]
    ew[neg] = -ew[neg]
    star = torch.zeros(200, 200)
    star[0, 1:] = star[1:, 0] = torch.linspace(0.1, 0.9, 199)
    idx = star.nonzero().t()
    ei, ew = torch.cat([ei, idx + 656], 1), torch.cat([ew, star[idx[0], idx[1]]])
    batch = torch.cat([batch, torch.full((200,), 4), torch.full((150,), 5)])
    return sizes + [200, 150], ei, ew, batch


@functools.lru_cache(maxsize=None)
def fixed_reference(name, k, T):
    _, ei, ew, batch = fixed_problem(name, k)
    kw = dict(seed=3, tol=0.0, max_iter=T)
    return (R.nmf_select(ei, k, ew, batch, dtype=torch.float64, **kw),
            R.nmf_select(ei, k, ew, batch, dtype=torch.float32, ordered=True, **kw))


@pytest.mark.parametrize("home", ["auto", "hbm"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("k", [2, 5, 32])
def test_fixed_iteration_counts_against_float64(k, T, home):
    """Raw W and H^T after exactly T iterations.  The bound per graph is the project's own (tests/test_gpu_nmf.py): 4 x the
    error of the fp32 ``ordered=True`` restatement against float64 on the same input plus 1e-6, never a number measured
    on the kernel.  ``auto`` goes through ``nmf_select`` (factors in LDS, in HBM past ``nmf_rows_lds_nodes``), ``hbm``
    through ``kernels.nmf_rows_factorize(home="hbm")`` on the small sizes.  The measured ratios kernel error / fp32
    restatement error are recorded in profiles/nmf_rows_forward.txt."""
    for name in (("small", "large") if home == "auto" else ("small",)):
        sizes, ei, ew, batch = fixed_problem(name, k)
        f64, f32 = fixed_reference(name, k, T)
        if home == "auto":
            fac = select(ei, ew, batch, k, seed=3, tol=0.0, max_iter=T, return_factors=True)[1]
        else:
            fac = rows_direct(ei, ew, batch, k, home="hbm", seed=3, tol=0.0, max_iter=T)
            assert fac["status"] == 0
        assert fac["iters"].cpu().tolist() == f64["iters"]
        lo = 0
        for m in sizes:
            for which in ("w", "ht"):
                ref = f64[which][lo:lo + m]
                own = float((f32[which][lo:lo + m].double() - ref).abs().max())
                err = float((fac[which][lo:lo + m].cpu().double() - ref).abs().max())
                print(f"nmf rows k={k} T={T} {home} n={m} {which}: kernel err {err:.3e}, fp32 restatement err {own:.3e}, "
                      f"ratio {err / max(own, 1e-30):.2f}")
                assert err <= 4.0 * own + 1e-6, (m, which, err, own)
            lo += m


# ------------------------------------------------------------------------------------------------ the stopping rule
def test_the_stopping_rule_leaves_at_the_first_iteration_under_tol():
    ei, ew, _ = R.planted_graphs([[50, 50, 50, 50]], 7)
    tol, cap = 1e-4, 5000
    so, fac = select(ei, ew, None, 4, tol=tol, max_iter=cap, return_factors=True)
    it = int(fac["iters"][0])
    assert 1 < it < cap and float(fac["ratio"][0]) <= tol
    so2, fac2 = select(ei, ew, None, 4, tol=0.0, max_iter=it, return_factors=True)
    assert torch.equal(fac2["w"], fac["w"]) and torch.equal(fac2["ht"], fac["ht"]) and torch.equal(so2.s, so.s)
    fac3 = select(ei, ew, None, 4, tol=tol, max_iter=it - 1, return_factors=True)[1]
    assert int(fac3["iters"][0]) == it - 1 and float(fac3["ratio"][0]) > tol


# ------------------------------------------------------------------------------------------------ routes of one batch
def test_every_native_route_in_one_batch():
    """The LDS kernel (20, 30), the new kernel with factors in LDS (129) and in HBM (one node past the frame), and a
    graph without nodes: rows in node order, the same bits on a second call and at another place in another batch."""
    from tgp import kernels as K
    k = 32
    sizes = [20, 129, 0, 30, K.nmf_rows_lds_nodes(k) + 1]
    ei, ew, batch = random_batch(sizes, 14)  # (graph 2 has no nodes)
    kw = dict(seed=5, tol=0.0, max_iter=3)
    ref = R.nmf_select(ei, k, ew, batch, dtype=torch.float64, **kw)
    so, fac = select(ei, ew, batch, k, return_factors=True, **kw)
    torch.testing.assert_close(so.s.cpu().double(), ref["s"], **TOL)
    assert fac["iters"].cpu().tolist() == ref["iters"] == [0, 3, 0, 0, 3]
    assert torch.equal(select(ei, ew, batch, k, **kw).s, so.s)
    mine = batch[ei[0]] == 1
    ei2, ew2, batch2 = random_batch([40], 15)
    moved = select(torch.cat([ei[:, mine] - 20, ei2 + 129], 1), torch.cat([ew[mine], ew2]),
                   torch.cat([torch.zeros(129, dtype=torch.long), batch2 + 1]), k, **kw).s
    assert torch.equal(moved[:129], so.s[20:149])


# ------------------------------------------------------------------------------------------------ declines and refusals
@functools.lru_cache(maxsize=None)
def declined_problem(kind):
    ei, ew, batch = random_batch([130, 20], 16)
    mine = (batch[ei[0]] == 0).nonzero().view(-1)
    if kind == "permuted":  # the first graph's edges in reverse: no group ascends
        order = torch.cat([mine.flip(0), torch.arange(mine.numel(), ei.size(1))])
    else:  # one edge twice
        order = torch.cat([torch.arange(8), torch.arange(7, ei.size(1))])
    return ei[:, order], ew[order], batch


@pytest.mark.parametrize("kind", ["permuted", "duplicate"])
def test_a_list_that_is_not_coalesced_is_declined_and_composed(kind):
    from tgp import kernels as K
    ei, ew, batch = declined_problem(kind)
    kw = dict(seed=2, tol=0.0, max_iter=3)
    out = rows_direct(ei, ew, batch, 3, sentinel=-7.0, **kw)
    s = out["s"].cpu()
    assert out["status"] == K.NMF_NOT_COALESCED and bool((s[:130] == -7.0).all()) and bool((s[130:] >= 0).all())
    assert out["iters"].cpu().tolist() == [0, 3]
    ref = R.nmf_select(ei, 3, ew, batch, dtype=torch.float64, **kw)
    so, fac = select(ei, ew, batch, 3, return_factors=True, **kw)
    torch.testing.assert_close(so.s.cpu().double(), ref["s"], **TOL)
    assert fac["iters"].cpu().tolist() == [3, 3]


@pytest.mark.parametrize("kind", ["nan", "two graphs"])
def test_refused_lists_raise(kind):
    ei, ew, batch = random_batch([130, 20], 17)
    ei, ew = ei.clone(), ew.clone()
    if kind == "nan":
        ew[5] = float("nan")
    else:
        ei[1, 5] = 140
    with pytest.raises(ValueError, match="NaN or infinity" if kind == "nan" else "two graphs"):
        select(ei, ew, batch, 3)


# ------------------------------------------------------------------------------------------------ memory
def test_a_warm_call_stays_below_one_dense_adjacency():
    from tgp.select import nmf_select
    d = dev()
    ei, ew, _ = random_batch([2048], 18)
    ei, ew = ei.to(d), ew.to(d)
    nmf_select(ei, 8, ew, tol=0.0, max_iter=2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    so = nmf_select(ei, 8, ew, tol=0.0, max_iter=2)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"nmf rows warm call on 2048 nodes: peak rise {rise} bytes against {2048 * 2048 * 4} of a dense adjacency")
    assert tuple(so.s.shape) == (2048, 8) and rise < 2048 * 2048 * 4
