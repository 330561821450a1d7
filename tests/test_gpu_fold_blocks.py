"""The block-order slabs of the dense poolers' two-launch route (gemm_mfma.h MODE 4 tail -> post_rows_kernel<true>).

The folded tail leaves S_r^T U_r and S_r^T X_r as arrays of 16 x 16 blocks in the accumulator layout of
v_mfma_f32_16x16x4_f32 -- element (p, c) in block (p / 16, c / 16) at word 4 lane + r, lane = 16 ((p % 16) / 4) + c % 16,
r = p % 4 -- and post_rows_kernel reads them back through the inverse map.  What can go wrong: a lane, row or block
swapped on either side; the diagonal test, which moved from float4 columns to float4 rows; a word of a partial block
(K, F multiples of 4 but not of 16) or of a block that is not stored reaching an output or a column sum; the degree
vector's adds taken in another order; a workspace sized for the row-major footprint.

Adds to test_gpu_dense_fold.py and test_gpu_fold_tail.py.  Every call goes through the C entry with a workspace this
file owns and fills with NaN first, is made twice and must repeat itself bit for bit.
Reference: dense_conn.py:111-122, base_reduce.py:158-161, utils/ops.py:282-335."""
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

RTOL = ATOL = 1e-5  # the reference's own fp32 tolerance
TILE = 128
# (B, N): the smallest batches that pass the gate of 256 row tiles, and eight slabs with a partial last tile
SWEEP_SHAPE = (256, 128)
KS, FS = (68, 100, 116, 128), (0, 4, 20, 60, 64)
GRID = [SWEEP_SHAPE + (k, f) for k in KS for f in FS]
MAP_CASES = [(256, 128, 128, 64), (256, 128, 100, 60), (128, 256, 128, 64), (128, 256, 68, 4), (32, 928, 128, 64),
             (32, 928, 116, 20)]
COLSUM_CASES = [(256, 128, 128), (128, 256, 100), (32, 928, 116)]


def _ids(case):
    return "-".join(f"{n}{v}" for n, v in zip("BNKF", case))


def _ceil16(v):
    return (v + 15) // 16 * 16


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _call_twice(S, A, X, flags, want_raw, want_post):
    """tgp_dense_pool_f32 on device tensors with a NaN-filled workspace of the size the library asks for; made twice.
    Returns (x_pool, adj_raw, adj_pool) on the host."""
    from tgp import _native as N
    from tgp import kernels
    L = N.lib()
    dev = S.device
    B, Nn, K = S.shape
    F = 0 if X is None else X.size(2)
    nbytes = L.tgp_dense_pool_workspace_bytes(B, Nn, K, F)
    outs = []
    for _ in range(2):
        ws = torch.full(((nbytes + 3) // 4,), float("nan"), dtype=torch.float32, device=dev)
        x_pool = torch.empty(B, K, F, device=dev) if F else None
        raw = torch.empty(B, K, K, device=dev) if want_raw else None
        post = torch.empty(B, K, K, device=dev) if want_post else None
        rc = L.tgp_dense_pool_f32(N.ptr(S), N.ptr(A), N.ptr(X), B, Nn, K, F, flags, kernels.ops_eps(), None, N.ptr(x_pool),
                                  N.ptr(raw), N.ptr(post), N.ptr(ws), nbytes, N.stream_ptr(dev))
        assert rc == 0, L.tgp_last_error()
        torch.cuda.synchronize()
        outs.append([None if t is None else t.cpu() for t in (x_pool, raw, post)])
    for u, v in zip(*outs):
        if u is not None:
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "two calls on the same inputs differ"
    return outs[0]


# ---- the address map on both sides ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _coded(B, N, K, F):
    """One-hot S with cluster(n) = n mod K; A and X hold, for every element (p, c) of S^T A S and (p, f) of S^T X, the
    element's own code p * width + column + 1 at exactly one place (which one depends on the graph), zeros elsewhere: the
    products are the code matrices, every element a distinct integer below 2^24."""
    S = torch.nn.functional.one_hot(torch.arange(N) % K, K).float().expand(B, N, K).contiguous()
    b = torch.arange(B).view(B, 1, 1)
    p = torch.arange(K).view(1, K, 1)
    reps = (N - 1 - torch.arange(K)) // K + 1  # nodes per cluster
    c = torch.arange(K).view(1, 1, K)
    i = p + K * ((p + c + b) % reps.view(1, K, 1))
    j = c + K * ((3 * p + c + 5 * b) % reps.view(1, 1, K))
    code_a = (p * K + c + 1).expand(B, K, K).float()
    A = torch.zeros(B, N, N)
    A[b.expand(B, K, K), i, j] = code_a
    X = code_x = None
    if F:
        f = torch.arange(F).view(1, 1, F)
        ix = p + K * ((p + f + b) % reps.view(1, K, 1))
        code_x = (p * F + f + 1).expand(B, K, F).float()
        X = torch.zeros(B, N, F)
        X[b.expand(B, K, F), ix, f.expand(B, K, F)] = code_x
    return S, A, X, code_a.contiguous(), code_x


@gpu
@pytest.mark.parametrize("want_raw", [True, False], ids=["raw", "no-raw"])
@pytest.mark.parametrize("rsl", [False, True], ids=["keep-loops", "remove-loops"])
@pytest.mark.parametrize("case", MAP_CASES, ids=_ids)
def test_every_element_arrives_at_its_own_place(dev, case, rsl, want_raw):
    """A swapped lane, row or block on either side of the slabs shows as a wrong integer at a known place."""
    from tgp import kernels
    S, A, X, code_a, code_x = _coded(*case)
    B, N, K, F = case
    assert code_a.max() < 2 ** 24 and torch.equal(torch.bmm(S.transpose(1, 2), torch.bmm(A, S)), code_a)
    flags = kernels.dense_flags(rsl, False, True, False)
    x_pool, raw, post = _call_twice(S.to(dev), A.to(dev), X.to(dev), flags, want_raw, True)
    if want_raw:
        wrong = (raw != code_a).nonzero()
        assert not len(wrong), f"adj_raw: {len(wrong)} wrong, first (b, p, c) = {wrong[0].tolist()}"
    else:
        assert raw is None
    want = code_a.clone()
    if rsl:
        want.diagonal(dim1=1, dim2=2).zero_()
    wrong = (post != want).nonzero()
    assert not len(wrong), f"adj_pool: {len(wrong)} wrong, first (b, p, c) = {wrong[0].tolist()}"
    wrong = (x_pool != code_x).nonzero()
    assert not len(wrong), f"x_pool: {len(wrong)} wrong, first (b, p, f) = {wrong[0].tolist()}"


# ---- partial blocks ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _adjacency(B, N):
    g = torch.Generator().manual_seed(91 * B + N)
    A = (torch.rand(B, N, N, generator=g) < 0.01).float()
    return torch.maximum(A, A.transpose(1, 2))


@functools.lru_cache(maxsize=None)
def _weighted_adjacency(B, N):
    g = torch.Generator().manual_seed(17 * B + N)
    return _adjacency(B, N) * (torch.rand(B, N, N, generator=g) + 0.1)


@functools.lru_cache(maxsize=None)
def _one_hot(B, N, K):
    g = torch.Generator().manual_seed(1000 * B + N + 7 * K)
    return torch.nn.functional.one_hot(torch.randint(0, K, (B, N), generator=g), K).float()


@functools.lru_cache(maxsize=None)
def _softmax(B, N, K):
    g = torch.Generator().manual_seed(3000 * B + N + 7 * K)
    return torch.softmax(torch.randn(B, N, K, generator=g), -1)


@functools.lru_cache(maxsize=None)
def _u64(kind, B, N, K):
    if kind == "binary":
        return torch.bmm(_adjacency(B, N).double(), _one_hot(B, N, K).double())
    return torch.bmm(_weighted_adjacency(B, N).double(), _softmax(B, N, K).double())


@pytest.fixture(scope="module")
def device_a(dev):
    cache = {}

    def get(kind, B, N):
        if (kind, B, N) not in cache:
            cache[(kind, B, N)] = (_adjacency if kind == "binary" else _weighted_adjacency)(B, N).to(dev)
        return cache[(kind, B, N)]
    return get


@gpu
@pytest.mark.parametrize("case", GRID, ids=_ids)
def test_partial_blocks_binary_is_exact(dev, device_a, case):
    """One-hot S, 0/1 A, small-integer X: the integer result, and no NaN of the workspace in any output."""
    from tgp import kernels
    B, N, K, F = case
    S = _one_hot(B, N, K)
    g = torch.Generator().manual_seed(4000 * B + N + 7 * F)
    X = torch.randint(-3, 4, (B, N, F), generator=g).float() if F else None
    flags = kernels.dense_flags(True, False, True, False)
    x_pool, raw, post = _call_twice(S.to(dev), device_a("binary", B, N), None if X is None else X.to(dev), flags, True, True)
    St = S.double().transpose(1, 2)
    raw_ref = torch.bmm(St, _u64("binary", B, N, K))
    assert torch.equal(raw.double(), raw_ref)
    raw_ref.diagonal(dim1=1, dim2=2).zero_()
    assert torch.equal(post.double(), raw_ref)
    if F:
        assert torch.equal(x_pool.double(), torch.bmm(St, X.double()))
    else:
        assert x_pool is None


@gpu
@pytest.mark.parametrize("rsl", [False, True], ids=["keep-loops", "remove-loops"])
@pytest.mark.parametrize("case", GRID, ids=_ids)
def test_partial_blocks_against_float64(dev, device_a, case, rsl):
    """Softmax S and weighted A against float64 through the degree-normalised output; everything finite."""
    import tgp_oracle as O
    from tgp import kernels
    B, N, K, F = case
    S = _softmax(B, N, K)
    g = torch.Generator().manual_seed(5000 * B + N + 7 * F)
    X = torch.randn(B, N, F, generator=g) if F else None
    flags = kernels.dense_flags(rsl, True, True, False)
    x_pool, raw, post = _call_twice(S.to(dev), device_a("weighted", B, N), None if X is None else X.to(dev), flags, True, True)
    St = S.double().transpose(1, 2)
    raw_ref = torch.bmm(St, _u64("weighted", B, N, K))
    for got, ref in ((raw, raw_ref), (post, O.postprocess_dense(raw_ref, rsl, True, True, False))) + \
            (((x_pool, torch.bmm(St, X.double())),) if F else ()):
        assert torch.isfinite(got).all(), "a word that is not part of the result reached an output"
        torch.testing.assert_close(got.double(), ref, rtol=RTOL, atol=ATOL)


@gpu
@pytest.mark.parametrize("case", [(256, 128, 100, 20), (256, 128, 68, 60)], ids=_ids)
def test_a_nan_in_x_stays_in_its_column(dev, device_a, case):
    """One NaN in X, in a row that is in range: x_pool carries it where the reference does and nowhere else."""
    from tgp import kernels
    B, N, K, F = case
    S = _one_hot(B, N, K)
    g = torch.Generator().manual_seed(6000 * B + N + 7 * F)
    X = torch.randint(-3, 4, (B, N, F), generator=g).float()
    X[3, N - 2, F - 1] = float("nan")
    X[5, 17, 0] = float("nan")
    x_pool, raw, post = _call_twice(S.to(dev), device_a("binary", B, N), X.to(dev), kernels.dense_flags(True, False, True, False),
                                    True, True)
    ref = torch.bmm(S.double().transpose(1, 2), X.double())
    assert torch.isnan(ref).sum() == 2 * K  # (0 * NaN: the whole column of that graph)
    assert torch.equal(torch.isnan(x_pool), torch.isnan(ref))
    assert torch.equal(torch.nan_to_num(x_pool.double()), torch.nan_to_num(ref))
    assert torch.isfinite(raw).all() and torch.isfinite(post).all()


# ---- the degree vector's summation order ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _scaled(B, N, K):
    """One-hot S and a 0/1 A whose rows carry a power of two that depends on the row tile and on the 16-row group of the
    row's cluster: every element of a slab is that weight times a count (exact in fp32), and the column-sum partials
    differ by orders of magnitude (2^-10 .. 2^10, as 1e-3 .. 1e3) between 16-row groups and between tiles."""
    S = _one_hot(B, N, K)
    cluster = S.argmax(-1)  # [B, N]
    tile = (torch.arange(N) // TILE).view(1, N)
    expo = torch.tensor([10.0, -10.0, 0.0, 4.0, -7.0])[(cluster // 16 + 2 * tile) % 5]
    return S, _adjacency(B, N) * torch.exp2(expo).unsqueeze(-1)


def _nested_fp32(slabs, rsl, eps):
    """The kernels' order on the host in fp32.  slabs [B, T, K, K] (exact).  Column sums: per tile and 16-row group the
    rows in order from 0, the eight groups of a tile in order from 0, the tiles in order from 0; R = slabs added in tile
    order; out = (R1 / d_j) / d_i with d = sqrt(max(colsum, eps))."""
    s = slabs.numpy().astype(np.float32)
    B, T, K, _ = s.shape
    zero_diag = s.copy()
    if rsl:
        idx = np.arange(K)
        zero_diag[:, :, idx, idx] = 0.0
    col = np.zeros((B, K), np.float32)
    for t in range(T):
        tot = np.zeros((B, K), np.float32)
        for q in range(8):
            part = np.zeros((B, K), np.float32)
            for r in range(16 * q, 16 * q + 16):
                part = part + (zero_diag[:, t, r, :] if r < K else np.float32(0.0))
            tot = tot + part
        col = col + tot
    d = np.sqrt(np.maximum(col, np.float32(eps)))
    R = s[:, 0].copy()
    for t in range(1, T):
        R = R + s[:, t]
    R1 = R.copy()
    if rsl:
        idx = np.arange(K)
        R1[:, idx, idx] = 0.0
    out = (R1 / d[:, None, :]) / d[:, :, None]
    assert R.dtype == np.float32 and out.dtype == np.float32 and d.dtype == np.float32
    return torch.from_numpy(R), torch.from_numpy(out)


@gpu
@pytest.mark.parametrize("rsl", [False, True], ids=["keep-loops", "remove-loops"])
@pytest.mark.parametrize("case", COLSUM_CASES, ids=lambda c: "-".join(f"{n}{v}" for n, v in zip("BNK", c)))
def test_degree_order_bit_for_bit(dev, case, rsl):
    """The degree-normalised output equals the nested order evaluated on the host in fp32, bit for bit: a reordered
    add, a row >= K of a partial block or the diagonal under self-loop removal that counts, shows."""
    from tgp import kernels
    B, N, K = case
    S, A = _scaled(B, N, K)
    T = (N + TILE - 1) // TILE
    U = torch.bmm(A.double(), S.double())
    slabs = torch.stack([torch.bmm(S[:, TILE * t:TILE * (t + 1)].double().transpose(1, 2), U[:, TILE * t:TILE * (t + 1)])
                         for t in range(T)], 1)
    assert torch.equal(slabs.float().double(), slabs)  # (exact in fp32)
    R, want = _nested_fp32(slabs.float(), rsl, kernels.ops_eps())
    magnitudes = slabs.sum(2)  # per-tile column sums
    assert (magnitudes.amax((1, 2)) / magnitudes.clamp_min(1e-30).amin((1, 2)) > 1e4).any()
    _, raw, post = _call_twice(S.to(dev), A.to(dev), None, kernels.dense_flags(rsl, True, True, False), True, True)
    assert torch.equal(raw.view(torch.int32), R.view(torch.int32))
    wrong = (post.view(torch.int32) != want.view(torch.int32)).nonzero()
    assert not len(wrong), f"{len(wrong)} elements differ in bits, first (b, p, c) = {wrong[0].tolist()}"


# ---- workspace size (no GPU) ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [SWEEP_SHAPE, (128, 256), (32, 928)], ids=lambda s: f"B{s[0]}-N{s[1]}")
def test_workspace_covers_the_block_order_footprint(shape):
    """tgp_dense_pool_workspace_bytes is at least what the folded route's block-order slabs take (K and F rounded up to
    16, one slab of each set per 128-row tile) plus one row of degree partials per tile."""
    from tgp import _native as N
    L = N.lib()
    B, Nn = shape
    tiles = (Nn + TILE - 1) // TILE
    for K in KS:
        for F in FS:
            k16, f16 = _ceil16(K), _ceil16(F)
            need = 4 * B * tiles * (k16 * k16 + k16 * f16 + K)
            assert L.tgp_dense_pool_workspace_bytes(B, Nn, K, F) >= need, (B, Nn, K, F)
