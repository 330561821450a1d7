"""The 16-bit storage kernels (csrc/sparse_half.hip) through the public operators: bf16 / fp16 rows are read and written
where they lie, and the result has THE BYTES of the upcast route ``op(x.float()).to(dtype)`` -- forward and gradient.

Against float64 the bound is derived, not chosen: rounding an fp32 value v to the storage type moves it by at most half
an ulp of the storage type at |v|, and |v| <= |ref| + e32 where e32 is the fp32 route's own error against the same float64
reference, measured in the same test; so |half - ref| <= ulp(|ref| + e32) / 2 + e32.  Min and max are exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16]
WIDTHS = [1, 7, 8, 24, 136, 2056]  # below a lane, the scalar route, one load, 3 lanes of a 4-group, 17 lanes, > 256 lanes
PADS = [0, 8, 1]  # contiguous rows, a row stride of F + 8 (still 16-byte loads) and of F + 1 (the scalar route)
ALL4 = ["sum", "mean", "min", "max"]
MEMBERS = [0, 1, 9, 300]  # supernodes: no member, one, one past the eight rows in flight, many rounds


def rows(n, F, pad, dtype, seed=0, nan_row=None):
    """[n, F] rows of `dtype` with row stride F + pad; rows 5..8 repeat row 4, so every extreme there is tied."""
    base = torch.randn(n, F + pad, generator=torch.Generator().manual_seed(seed))
    if n > 8:
        base[5:9] = base[4]
    if nan_row is not None:
        base[nan_row] = float("nan")
    return base.to(DEV, dtype)[:, :F]


def half_ulp(v, dtype):
    """Half an ulp of `dtype` at the magnitudes `v` (float64)."""
    bits, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    exponent = (torch.frexp(v)[1] - 1).clamp(min=emin).long()
    return ((exponent - bits - 1 + 1023) << 52).view(torch.float64)  # the exact power of two (a device pow is not)


def compare(half, up32, ref64, dtype, nan=False, exact=False):
    want = up32.to(dtype)
    assert half.dtype == dtype and half.shape == want.shape
    keep = ~torch.isnan(want) if nan else torch.ones_like(want, dtype=torch.bool)
    assert torch.equal(torch.isnan(half), torch.isnan(want))
    assert torch.equal(half.view(torch.int16)[keep], want.view(torch.int16)[keep])
    e32 = (up32.double() - ref64).abs()[keep]
    err = (half.double() - ref64).abs()[keep]
    assert bool((err <= half_ulp(ref64.abs()[keep] + e32, dtype) + e32).all()), float(err.max())
    if exact:
        assert torch.equal(half.double()[keep], ref64[keep])


def check_routes(fn, ref, x, dtype, grads=True, nan=False, exact=False):
    """`fn` on the half rows, on their fp32 copy (the upcast route) and `ref` in float64: outputs, then the gradients
    of a fixed upstream gradient."""
    xs = [x.detach().requires_grad_(grads), x.detach().float().requires_grad_(grads),
          x.detach().double().requires_grad_(grads)]
    outs = [fn(xs[0]), fn(xs[1]), ref(xs[2])]
    compare(outs[0].detach(), outs[1].detach(), outs[2].detach(), dtype, nan, exact)
    if grads and outs[2].numel() > 0:
        g = torch.randn(outs[2].shape, generator=torch.Generator().manual_seed(7)).to(DEV, dtype)
        gh, g32, g64 = (torch.autograd.grad(o, xi, g.to(o.dtype))[0] for o, xi in zip(outs, xs))
        compare(gh, g32, g64, dtype, nan)


def assignment(dtype=None):
    """Supernodes of MEMBERS sizes over shuffled node ids, weighted; with `dtype` the weights are stored in it."""
    from tgp.select import SelectOutput
    g = torch.Generator().manual_seed(11)
    cluster = torch.repeat_interleave(torch.arange(len(MEMBERS)), torch.tensor(MEMBERS))
    n = cluster.numel() + 6
    node = torch.randperm(n, generator=g)[:cluster.numel()].sort().values
    w = torch.rand(cluster.numel(), generator=g) + 0.5
    w = w if dtype is None else w.to(dtype)
    so = SelectOutput(cluster_index=cluster.to(DEV), node_index=node.to(DEV), weight=w.to(DEV), num_nodes=n,
                      num_supernodes=len(MEMBERS))
    return so, n, node.to(DEV), cluster.to(DEV), w.to(DEV).double().view(-1, 1)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_and_lift(dtype, F, pad):
    from tgp.lift import BaseLift
    from tgp.reduce import BaseReduce
    so, n, node, cluster, w = assignment()
    K = len(MEMBERS)
    for nan_row in (None, int(node[3])):
        check_routes(lambda x: BaseReduce()(x, so)[0],
                     lambda x: torch.zeros(K, F, dtype=x.dtype, device=DEV).index_add_(0, cluster, x[node] * w),
                     rows(n, F, pad, dtype, 1, nan_row), dtype, nan=nan_row is not None)
    check_routes(lambda xp: BaseLift(matrix_op="transpose")(xp, so),
                 lambda xp: torch.zeros(n, F, dtype=xp.dtype, device=DEV).index_add_(0, node, xp[cluster] * w),
                 rows(K, F, pad, dtype, 2), dtype)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_to_one_reduce(dtype, F, pad):
    from tgp import kernels as K
    g = torch.Generator().manual_seed(5)
    n, k = 70, 37  # two workgroups' worth of groups at F = 2056, a ragged last round of four
    node = torch.randperm(n, generator=g)[:k].sort().values.to(DEV)
    cluster = torch.randperm(k, generator=g).to(DEV)
    w = (torch.rand(k, generator=g) - 0.5).to(DEV)
    index = K.one_to_one_index(node, cluster, w)
    x = rows(n, F, pad, dtype, 3)
    ref = torch.zeros(k, F, dtype=torch.float64, device=DEV).index_add_(0, cluster, x.double()[node] * w.double().view(-1, 1))
    compare(K.reduce_sparse_h16(x, node, w, index), K.reduce_sparse(x.float(), node, w, index), ref, dtype)


def readout_ref(vals, idx, G, ops):
    F = vals.size(1)
    total = torch.zeros(G, F, dtype=vals.dtype, device=DEV).index_add_(0, idx, vals)
    count = torch.bincount(idx, minlength=G).clamp(min=1).view(-1, 1)
    ext = {op: torch.stack([getattr(vals[idx == g], "a" + op)(0) if bool((idx == g).any()) else vals.new_zeros(F)
                            for g in range(G)]) for op in ("min", "max") if op in ops}
    return torch.cat([total if op == "sum" else total / count if op == "mean" else ext[op] for op in ops], dim=-1)


def reduce_op(ops):
    from tgp.reduce import GlobalReduce
    return GlobalReduce(ops[0]) if len(ops) == 1 else GlobalReduce("multi", aggrs=list(ops))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_readout_over_segments(dtype, F, pad):
    """Segments on both sides of the split route: up to 256 rows the items write the output, one of 257 or more sends
    the batch through the fp32 partial records and the fold."""
    for lens in ([0, 1, 255, 256], [0, 1, 255, 256, 257, 700]):
        batch = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens)).to(DEV)
        x = rows(batch.numel(), F, pad, dtype, 4)
        for ops in (["sum"], ["mean"], ["min"], ["max"], ALL4):
            check_routes(lambda t: reduce_op(ops)(t, batch=batch, size=len(lens)),
                         lambda t: readout_ref(t, batch, len(lens), ops), x, dtype, exact=ops in (["min"], ["max"]))
    # (GlobalReduce keeps min / max over the 700-row batch on the upcast route: the kernel's split route, called directly)
    from tgp import kernels as K
    ptr = torch.tensor([0, 0, 1, 256, 512, 769, 1469], device=DEV)
    half, up = (call(t, K.segment_ops_mask(ALL4), 6, 700, ptr=ptr, want_aux=True)
                for call, t in ((K.segment_aggr_h16, x), (K.segment_aggr, x.float())))
    compare(half[0], up[0], readout_ref(x.double(), batch, 6, ALL4), dtype)
    assert torch.equal(half[1], up[1]) and torch.equal(half[2], up[2])  # the tie counts and the group sizes


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_readout_dense_masked_and_gathered(dtype, F):
    from tgp.reduce import AggrReduce, get_aggr
    mask = torch.rand(3, 40, generator=torch.Generator().manual_seed(9)) < 0.7
    mask[1] = False  # an empty graph
    mask = mask.to(DEV)
    idx = torch.arange(3, device=DEV).repeat_interleave(40)[mask.view(-1)]
    x = rows(120, F, 0, dtype, 6)
    for ops in (["sum"], ["mean"], ["min"], ["max"], ALL4):
        check_routes(lambda t: reduce_op(ops)(t.view(3, 40, F), mask=mask),
                     lambda t: readout_ref(t[mask.view(-1)], idx, 3, ops), x, dtype)
    so, n, node, cluster, w = assignment(dtype)  # the gathered source: x[node] * weight, weights stored in `dtype` too
    xg = rows(n, F, 0, dtype, 8)
    for ops in (["sum"], ALL4):
        aggr = get_aggr(ops[0]) if len(ops) == 1 else get_aggr("multi", aggrs=list(ops))
        check_routes(lambda t: AggrReduce(aggr)(t, so)[0], lambda t: readout_ref(t[node] * w, cluster, len(MEMBERS), ops),
                     xg, dtype, grads=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_groups_no_rows_and_overflow(dtype):
    from tgp import kernels as K
    from tgp.reduce.aggr import SumAggregation
    x = rows(12, 8, 0, dtype)
    none = torch.zeros(0, dtype=torch.long, device=DEV)
    for groups in (0, 3):  # zero rows into no group, and into three empty ones
        out = SumAggregation()(x[:0], index=none, dim_size=groups)
        assert out.dtype == dtype and out.shape == (groups, 8) and not bool(out.any())
        pooled = K.reduce_sparse_h16(x[:0], none, None, K.build_assign_index(none, groups))
        assert pooled.dtype == dtype and pooled.shape == (groups, 8) and not bool(pooled.any())
    if dtype == torch.float16:  # an fp32 sum past 65504 rounds to inf on both routes
        big = torch.full((2, 8), 60000.0, dtype=dtype, device=DEV)
        one = torch.zeros(2, dtype=torch.long, device=DEV)
        for out, up in ((SumAggregation()(big, index=one, dim_size=1), SumAggregation()(big.float(), index=one, dim_size=1)),
                        (K.reduce_sparse_h16(big, torch.arange(2, device=DEV), None, K.build_assign_index(one, 1)),
                         K.reduce_sparse(big.float(), torch.arange(2, device=DEV), None, K.build_assign_index(one, 1)))):
            assert bool(torch.isinf(out).all()) and torch.equal(out, up.to(dtype)) and bool((up == 120000.0).all())


def test_no_fp32_temporary():
    """A warm call on bf16 X [65536, 128] stays within the 8.4 MB of the Reduce's output (K = 32768) plus 1 MB -- the
    readout's 2 MB of fp32 partial records included -- where the upcast route holds a 33.5 MB fp32 copy of X."""
    from tgp import kernels as K
    from tgp.reduce import BaseReduce, GlobalReduce
    from tgp.select import SelectOutput
    n, k, F = 65536, 32768, 128
    x = torch.randn(n, F, device=DEV).bfloat16()
    node = torch.arange(0, n, 2, device=DEV)
    cluster = torch.randperm(k, device=DEV)
    so = SelectOutput(cluster_index=cluster, node_index=node, weight=torch.rand(k, device=DEV), num_nodes=n, num_supernodes=k)
    so._assign_index = K.one_to_one_index(so.node_index, so.cluster_index, so.weight)
    for call, out_bytes in ((lambda: BaseReduce()(x, so)[0], k * F * 2), (lambda: GlobalReduce("sum")(x), F * 2)):
        call()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = call()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        assert out.dtype == torch.bfloat16 and out.numel() * 2 == out_bytes and rise <= k * F * 2 + (1 << 20) < n * F * 4, rise


def test_public_classes_on_bf16():
    from tgp.poolers import SEPPooling, get_pooler
    from tgp.reduce import GlobalReduce
    g = torch.Generator().manual_seed(13)
    sizes = [30, 17, 25]
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes)).to(DEV)
    blocks, off = [], 0
    for n in sizes:
        a = torch.triu(torch.rand(n, n, generator=g) < 0.3, 1)
        blocks.append((a | a.t()).nonzero().t() + off)
        off += n
    ei = torch.cat(blocks, 1).to(DEV)
    x = torch.randn(off, 16, generator=g).to(DEV).bfloat16()
    bits = lambda t: t.view(torch.int16)
    topk = get_pooler("topk", in_channels=16, ratio=0.5).to(DEV).train()
    for pool in (topk, SEPPooling()):
        out, again, up = pool(x=x, adj=ei, batch=batch), pool(x=x, adj=ei, batch=batch), pool(x=x.float(), adj=ei, batch=batch)
        assert out.x.dtype == torch.bfloat16 and torch.equal(bits(out.x), bits(up.x.bfloat16()))
        assert torch.equal(bits(out.x), bits(again.x))
        lifted = pool(x=out.x, so=out.so, lifting=True)
        assert lifted.dtype == torch.bfloat16 and lifted.shape == x.shape
        assert torch.equal(bits(lifted), bits(pool(x=out.x.float(), so=up.so, lifting=True).bfloat16()))
        assert torch.equal(bits(lifted), bits(pool(x=out.x, so=out.so, lifting=True)))
    # the assignment weights' gradient keeps the upcast path (pair_dot has no 16-bit form): the same numbers as before
    from tgp.reduce.base_reduce import _SparseReduceFn
    so, n, node, cluster, _ = assignment()
    xr = rows(n, 24, 0, torch.bfloat16, 1)
    gr = torch.randn(len(MEMBERS), 24, generator=g).to(DEV).bfloat16()
    w = so.weight.detach().clone().requires_grad_(True)
    grads = [torch.autograd.grad(out, w, gr)[0] for out in (_SparseReduceFn.apply(xr, w, so),
                                                            _SparseReduceFn.apply(xr.float(), w, so).bfloat16())]
    assert torch.equal(grads[0], grads[1]) and bool(grads[0].any())
    multi = GlobalReduce("multi", aggrs=["sum", "mean", "max"])
    out = multi(x, batch=batch)
    assert out.dtype == torch.bfloat16 and out.shape == (3, 48)
    assert torch.equal(bits(out), bits(multi(x.float(), batch=batch).bfloat16())) and torch.equal(bits(out), bits(multi(x, batch=batch)))
