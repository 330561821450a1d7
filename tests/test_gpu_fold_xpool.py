"""x_pool = S^T X of the dense poolers' two-launch route, formed in the post-processing launch (dense_post.h,
post_rows_kernel<true>) instead of the folded tail of the first (gemm_mfma.h, MODE 4 under TGP_FOLD_X_LATE).

The post workgroup of 16 clusters forms its 16 x F block of x_pool itself: wave t multiplies tile t of N (128 rows) in
four chains of 32 v_mfma_f32_16x16x4_f32 from zero -- S_t^T as A, X_t as B, k-groups of four rows in ascending order --
with operands read straight from S and X, and the tiles' partials are added in tile order by one owner per element.
What can go wrong: a tile given to two waves or to none (one, two, five, eight tiles), rows of the last tile beyond N
that are not zeros (N = 520: eight rows), clusters beyond K or features beyond F of a partial 16-block that leak into
the result (K, F multiples of 4 but not of 16), a column of X that lands in another column of x_pool (the lanes' column
assignment is a permutation), partials added in another order, a NaN or Inf of X that spreads beyond its column, a tail
of the first launch that lost part of S^T U or of the degree partials when the X part left it.

Checks: (a) one-hot S and small-integer X: x_pool (and raw S^T A S) equal the integer result; (b) softmax S and random
X against float64 at the fp32 bar of test_gpu_fold_tail.py; (c) the tile order, bit for bit: one-hot S and X rows
scaled by a power of two per tile (2^-10 .. 2^10, reversed in odd graphs) make every per-tile partial exact in fp32, so
x_pool must be the fp32 sum of the partials in tile order and nothing else; (d) every call is made twice and repeats
itself bit for bit; (e) a NaN / an Inf in one column of X fills that column of x_pool and no other; (f) raw and the
degree-normalised adj_pool of the same calls against float64.  Both adjacency layouts; x_pool into a caller's buffer.

K = 20 and K = 64 are checked as well, but the folded route starts at K = 68 (its post-processing kernel takes
64 < K <= 128): the route test asserts two launches for K > 64 and that the smaller K do not reach this kernel.
Reference: base_reduce.py:158-161, dense_conn.py:111-122, utils/ops.py:282-335."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-5  # as tests/test_gpu_fold_tail.py (the reference's own fp32 tolerance)
TILE = 128
# (B, N): >= 256 row tiles, N <= 1024: one tile, two, five with a last tile of 8 rows, eight
SHAPES = [(256, 128), (128, 256), (64, 520), (32, 1024)]
KS, FS = (20, 64, 68, 100, 128), (4, 36, 64)
CASES = [SHAPES[0] + (k, f) for k in KS for f in FS]
CASES += [(128, 256, 128, 64), (128, 256, 68, 36), (128, 256, 20, 4), (128, 256, 64, 64),
          (64, 520, 128, 64), (64, 520, 100, 36), (64, 520, 64, 4), (64, 520, 20, 36),
          (32, 1024, 128, 64), (32, 1024, 100, 4), (32, 1024, 68, 64), (32, 1024, 20, 36)]
LAYOUTS = ("row-major", "k-major")


def _ids(case):
    return "B{}-N{}-K{}-F{}".format(*case)


@functools.lru_cache(maxsize=None)
def _adjacency(B, N):
    """0/1 adjacencies, ~2 % nonzeros, not symmetric."""
    g = torch.Generator().manual_seed(91 * B + N)
    return (torch.rand(B, N, N, generator=g) < 0.02).float()


@functools.lru_cache(maxsize=None)
def _weighted_a(B, N):
    g = torch.Generator().manual_seed(92 * B + N)
    return _adjacency(B, N) * (torch.rand(B, N, N, generator=g) + 0.1)


@functools.lru_cache(maxsize=None)
def _one_hot_s(B, N, K):
    g = torch.Generator().manual_seed(1100 * B + N + 7 * K)
    return torch.nn.functional.one_hot(torch.randint(0, K, (B, N), generator=g), K).float()


@functools.lru_cache(maxsize=None)
def _softmax_s(B, N, K):
    g = torch.Generator().manual_seed(3100 * B + N + 7 * K)
    return torch.softmax(torch.randn(B, N, K, generator=g), -1)


def _int_x(B, N, F):
    g = torch.Generator().manual_seed(4100 * B + N + 7 * F)
    return torch.randint(-3, 4, (B, N, F), generator=g).float()


def _real_x(B, N, F):
    g = torch.Generator().manual_seed(5100 * B + N + 7 * F)
    return torch.randn(B, N, F, generator=g)


@functools.lru_cache(maxsize=None)
def _raw64(kind, B, N, K):
    """float64 S^T (A S) of a batch (shared by the feature widths and the layouts)."""
    A, S = (_adjacency(B, N), _one_hot_s(B, N, K)) if kind == "binary" else (_weighted_a(B, N), _softmax_s(B, N, K))
    return torch.bmm(S.double().transpose(1, 2), torch.bmm(A.double(), S.double()))


def _xpool64(S, X):
    return torch.bmm(S.double().transpose(1, 2), X.double())


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def device_a(dev):
    """The adjacency of a shape on the device in either layout, uploaded once.  k-major: the memory holds A^T and the
    tensor is its transposed view, which the entry passes on as it lies (TGP_ADJ_TRANSPOSED)."""
    cache = {}

    def get(kind, B, N, layout):
        key = (kind, B, N, layout)
        if key not in cache:
            A = (_adjacency if kind == "binary" else _weighted_a)(B, N)
            if layout == "k-major":
                cache[key] = A.transpose(1, 2).contiguous().to(dev).transpose(1, 2)
                assert not cache[key].is_contiguous()
            else:
                cache[key] = A.to(dev)
        return cache[key]
    return get


def _call_twice(s, a, x, flags, want_raw, want_post, out_x=None):
    """(d) One call, made twice: the outputs on the host, having repeated themselves bit for bit."""
    from tgp import kernels
    outs = []
    for _ in range(2):
        if out_x is not None:
            out_x.fill_(float("nan"))
        out = kernels.dense_pool(s, a, x, flags, want_raw=want_raw, want_post=want_post, out_x=out_x)
        torch.cuda.synchronize()
        outs.append([None if t is None else t.cpu() for t in out])
    for u, v in zip(*outs):
        assert (u is None) == (v is None)
        if u is not None:
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "two calls on the same inputs differ"
    return outs[0]


def _check_against_f64(got, ref):
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert torch.equal(torch.isinf(got), torch.isinf(ref))
    torch.testing.assert_close(got.double(), ref, rtol=RTOL, atol=ATOL, equal_nan=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_binary_is_exact(dev, device_a, case, layout):
    """(a) One-hot S, 0/1 A, small-integer X: x_pool and raw S^T A S equal the integer computation on the host."""
    B, N, K, F = case
    S, X = _one_hot_s(B, N, K), _int_x(B, N, F)
    x_pool, raw, _ = _call_twice(S.to(dev), device_a("binary", B, N, layout), X.to(dev), 0, True, False)
    xp_ref, raw_ref = _xpool64(S, X), _raw64("binary", B, N, K)
    assert torch.equal(xp_ref, xp_ref.round()) and xp_ref.abs().max() < 2 ** 24
    bad = [b for b in range(B) if not torch.equal(x_pool[b].double(), xp_ref[b])]
    assert not bad, f"x_pool differs from the integer reference in graphs {bad[:8]} ({len(bad)} in all)"
    assert torch.equal(raw.double(), raw_ref)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_weighted_against_float64(dev, device_a, case, layout):
    """(b), (f) Softmax S, weighted A, random X against float64 at the fp32 bar: x_pool, raw, and the degree-normalised
    adj_pool against the oracle's post-processing of the float64 product (so the tail's column sums are part of the
    check); self loops removed in every other case."""
    import tgp_oracle as O
    from tgp import kernels
    B, N, K, F = case
    rsl = CASES.index(case) % 2 == 0
    S, X = _softmax_s(B, N, K), _real_x(B, N, F)
    flags = kernels.dense_flags(rsl, True, True, False)
    x_pool, raw, adj_pool = _call_twice(S.to(dev), device_a("weighted", B, N, layout), X.to(dev), flags, True, True)
    raw_ref = _raw64("weighted", B, N, K)
    _check_against_f64(x_pool, _xpool64(S, X))
    _check_against_f64(raw, raw_ref)
    _check_against_f64(adj_pool, O.postprocess_dense(raw_ref, rsl, True, True, False))


def _tile_scales(B, N):
    """[B, N]: 2^e of each row's tile, e spread over -10 .. 10 in tile order (one tile: 0), reversed in odd graphs."""
    T = (N + TILE - 1) // TILE
    exps = [0] if T == 1 else [round(-10 + 20 * t / (T - 1)) for t in range(T)]
    per_row = torch.tensor(exps, dtype=torch.float64).repeat_interleave(TILE)[:N]
    e = per_row.repeat(B, 1)
    e[1::2] = -e[1::2]
    return torch.pow(2.0, e).float()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", [c for c in CASES if c[2] > 64], ids=_ids)  # (the folded route: its order is pinned here)
def test_tile_order_bit_for_bit(dev, device_a, case, layout):
    """(c) Every per-tile partial S_t^T X_t is exact in fp32, so x_pool must be their fp32 sum in tile order, starting
    from tile 0's, bit for bit: another order, a pairwise tree or one chain over all of N rounds differently."""
    B, N, K, F = case
    S = _one_hot_s(B, N, K)
    g = torch.Generator().manual_seed(6100 * B + N + 7 * F)
    # (integers of seven bits: with the scales 20 binary places apart the sum of two partials does not fit fp32's 24)
    X = torch.randint(-100, 101, (B, N, F), generator=g).float() * _tile_scales(B, N)[:, :, None]
    x_pool, _, _ = _call_twice(S.to(dev), device_a("binary", B, N, layout), X.to(dev), 0, True, False)
    St = S.double().transpose(1, 2)
    parts = [torch.bmm(St[:, :, t:t + TILE], X[:, t:t + TILE].double()) for t in range(0, N, TILE)]
    assert all(torch.equal(p.float().double(), p) for p in parts), "a per-tile partial is not exact in fp32"
    want = parts[0].float() + 0.0  # (an empty cluster of a tile: the accumulators start from +0)
    for p in parts[1:]:
        want = want + p.float()
    if len(parts) > 1:
        mags = torch.stack(parts).abs()
        big = mags.amax(0)
        small = torch.where(mags > 0, mags, torch.full_like(mags, float("inf"))).amin(0)
        assert (big / small)[torch.isfinite(small)].max() > 1e4, "the partials of no element differ by more than 10^4"
        # (... and the sum rounds: a kernel that added the partials otherwise, or ran one chain over all of N, shows)
        assert not torch.equal(want.double(), sum(parts)), "the sum of the partials is exact in fp32: no order shows"
    assert torch.equal(x_pool.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("case", [(256, 128, 100, 36), (128, 256, 128, 64), (64, 520, 68, 4), (32, 1024, 128, 64)], ids=_ids)
def test_nonfinite_stays_in_its_column(dev, device_a, case, value):
    """(e) One NaN / +Inf in X (graph 1, a row of the last tile, column F - 3): with a strictly positive S that whole
    column of x_pool[1] is NaN / +Inf, every other value is finite and agrees with float64; raw is untouched."""
    B, N, K, F = case
    S, X = _softmax_s(B, N, K), _real_x(B, N, F).clone()
    col = F - 3
    X[1, N - 2, col] = value
    x_pool, raw, _ = _call_twice(S.to(dev), device_a("weighted", B, N, "row-major"), X.to(dev), 0, True, False)
    hit = torch.zeros(B, K, F, dtype=torch.bool)
    hit[1, :, col] = True
    bad = torch.isnan(x_pool) if value != value else (x_pool == float("inf"))
    assert torch.equal(bad, hit)
    assert torch.isfinite(x_pool[~hit]).all()
    ref = _xpool64(S, X)
    torch.testing.assert_close(x_pool[~hit].double(), ref[~hit], rtol=RTOL, atol=ATOL)
    _check_against_f64(raw, _raw64("weighted", B, N, K))


@pytest.mark.parametrize("case", [(256, 128, 100, 36), (32, 1024, 128, 64)], ids=_ids)
def test_x_pool_into_a_callers_buffer(dev, device_a, case):
    """x_pool written into the middle slot of a caller's [3, B, K, F] buffer: the bits of the call that allocates its
    own, and the neighbouring slots untouched."""
    B, N, K, F = case
    S, X = _softmax_s(B, N, K), _real_x(B, N, F)
    s, a, x = S.to(dev), device_a("weighted", B, N, "row-major"), X.to(dev)
    own, _, _ = _call_twice(s, a, x, 0, False, True)
    buf = torch.full((3, B, K, F), 7.0, device=dev)
    got, _, _ = _call_twice(s, a, x, 0, False, True, out_x=buf[1])
    assert torch.equal(got.view(torch.int32), own.view(torch.int32))
    assert torch.equal(buf[1].cpu().view(torch.int32), own.view(torch.int32))
    assert (buf[0] == 7.0).all() and (buf[2] == 7.0).all()
    _check_against_f64(own, _xpool64(S, X))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"B{b}-N{n}" for b, n in SHAPES])
def test_shapes_take_the_folded_route(dev, device_a, shape, K):
    """K > 64: two device kernels per call, the folded product and the post-processing launch that now forms x_pool.
    K <= 64 lies below the route's post-processing kernel and must not reach it."""
    from torch.profiler import ProfilerActivity, profile
    from tgp import kernels
    B, N = shape
    s, a, x = _one_hot_s(B, N, K).to(dev), device_a("binary", B, N, "row-major"), _int_x(B, N, 4).to(dev)
    kernels.dense_pool(s, a, x)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        kernels.dense_pool(s, a, x)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    if K > 64:
        assert len(names) == 2 and any("post_rows_kernel" in n for n in names), names
    else:
        assert not any("post_rows_kernel" in n for n in names), names
