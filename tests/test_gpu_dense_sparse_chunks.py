"""U = A S of the dense poolers' tiled path skips the MFMAs of A chunks that are mostly zeros (gemm_mfma.h, MODE 3):
every density, chunks of both kinds inside one tile, both adjacency layouts, tails, non-finite S, determinism and the
training forward.  Reference: dense_conn.py:111-122, base_reduce.py:158-161, utils/ops.py:282-335."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-5
# The skipping form runs when the 128 x 128 grid fills the chip (>= 256 tiles: 32 graphs at N = 1024, K = 128); smaller
# batches keep the plain MFMA kernel with the tile picker's smaller tiles.  Cases below are sized for the former unless
# they say otherwise.
B32 = 32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _inputs(B, N, K, F, seed):
    g = torch.Generator().manual_seed(seed)
    S = torch.softmax(torch.randn(B, N, K, generator=g), -1)
    X = torch.randn(B, N, F, generator=g)
    return S, X, g


def _adj(B, N, p, g, weights=None):
    A = (torch.rand(B, N, N, generator=g) < p).float()
    A = torch.maximum(A, A.transpose(1, 2))
    if weights is not None:
        A = A * weights
    return A


def _to_dev(A, dev, transposed):
    """A on the device, contiguous or as the transposed view DenseSRCPooling's preprocessing hands over (src.py:442-443)."""
    if transposed:
        return A.transpose(1, 2).contiguous().to(dev).transpose(1, 2)
    return A.to(dev)


def _check(S, A, X, dev, transposed=False, scale=1.0):
    """reduce_connect (raw and post-processed) and DenseConnect against the CPU oracle; values / scale compared."""
    import tgp_oracle as O
    from tgp.connect import DenseConnect
    from tgp.reduce import BaseReduce
    from tgp.select import SelectOutput
    from tgp.src import DenseSRCPooling
    so = SelectOutput(s=S.to(dev))
    Ad = _to_dev(A, dev, transposed)
    pool = DenseSRCPooling(reducer=BaseReduce(), connector=DenseConnect(), adj_transpose=True)
    x_pool, raw, adj_pool = pool.reduce_connect(X.to(dev), Ad, so, want_raw=True)
    raw_ref = O.dense_connect(S, A)
    torch.testing.assert_close(x_pool.cpu(), O.reduce_dense(S, X), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(raw.cpu() / scale, raw_ref / scale, rtol=RTOL, atol=ATOL)
    post_ref = O.postprocess_dense(raw_ref, True, True, True, False)
    torch.testing.assert_close(adj_pool.cpu(), post_ref, rtol=RTOL, atol=ATOL)
    conn = DenseConnect()
    torch.testing.assert_close(conn.dense_connect(adj=Ad, s=S.to(dev)).cpu() / scale, raw_ref / scale, rtol=RTOL,
                               atol=ATOL)
    out, _ = conn(Ad, so)
    torch.testing.assert_close(out.cpu(), post_ref, rtol=RTOL, atol=ATOL)


def _u(S, A, dev, transposed=False):
    """U = A S as the training forward writes it (tgp_dense_pool_train_fwd_f32, the _PoolLargeFn route)."""
    from tgp import _native as NN
    from tgp import kernels as K
    B, N, Kc = S.shape
    F = 4
    X = torch.zeros(B, N, F, device=dev)
    acat = torch.full((B, N, 3 * Kc + F + K.TRAIN_PAD), float("nan"), device=dev)
    Ad = _to_dev(A, dev, transposed)
    mem, flags = (Ad.transpose(1, 2), NN.ADJ_TRANSPOSED) if transposed else (Ad, 0)
    K.dense_pool_train_fwd(S.to(dev), mem, X, K.dense_flags(True, True, True, False) | flags, acat, False)
    return acat[:, :, :Kc].cpu()


@pytest.mark.parametrize("p", [0.0, 0.001, 0.02, 0.1, 0.3, 1.0])
def test_density_sweep(dev, p):
    S, X, g = _inputs(B32, 1024, 128, 64, seed=int(p * 1000) + 1)
    A = _adj(B32, 1024, p, g)
    _check(S, A, X, dev)


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("p", [0.02, 1.0])
def test_small_batches_keep_the_mfma_tiles(dev, B, p):
    S, X, g = _inputs(B, 1024, 128, 64, seed=B + int(p * 100))
    A = _adj(B, 1024, p, g)
    _check(S, A, X, dev)


@pytest.mark.parametrize("transposed", [False, True])
def test_mixed_chunks_in_one_tile(dev, transposed):
    """A dense column block next to a sparse remainder (whole k-steps of MFMAs beside skipped ones), and dense rows
    next to sparse rows: 8 dense rows of a 128-row tile leave its chunks under the threshold, 32 put them over it."""
    B, N, Kc, F = B32, 1024, 128, 64
    S, X, g = _inputs(B, N, Kc, F, seed=7)
    A = (torch.rand(B, N, N, generator=g) < 0.01).float()
    A[0, :, 64:192] = torch.rand(N, 128, generator=g)   # dense k-steps 2..5 of every row tile of graph 0
    A[1, 128:136, :] = torch.rand(8, N, generator=g)    # row tile 1 of graph 1: 8 dense rows (256 nonzeros a chunk)
    A[1, 512:544, :] = torch.rand(32, N, generator=g)   # row tile 4: 32 dense rows (1024 nonzeros a chunk)
    A[2, 5::128, :] = torch.rand(8, N, generator=g)     # one dense row in every row tile
    _check(S, A, X, dev, transposed)
    torch.testing.assert_close(_u(S, A, dev, transposed), torch.matmul(A, S), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("transposed", [False, True])
def test_mixed_batch(dev, transposed):
    B, N, Kc, F = B32, 1024, 128, 64
    S, X, g = _inputs(B, N, Kc, F, seed=8)
    A = torch.cat([_adj(1, N, (0.0, 0.002, 0.02, 0.15, 0.5, 1.0)[i % 6], g) for i in range(B)])
    _check(S, A, X, dev, transposed)


@pytest.mark.parametrize("kind", ["weighted", "negative", "small", "large"])
def test_values(dev, kind):
    B, N, Kc, F = B32, 1024, 128, 64
    S, X, g = _inputs(B, N, Kc, F, seed=9)
    w = {"weighted": torch.rand(B, N, N, generator=g) + 0.1,
         "negative": torch.randn(B, N, N, generator=g),
         "small": (torch.rand(B, N, N, generator=g) + 0.5) * 1e-20,
         "large": (torch.rand(B, N, N, generator=g) + 0.5) * 1e20}[kind]
    A = _adj(B, N, 0.02, g) * w
    scale = {"small": 1e-20, "large": 1e20}.get(kind, 1.0)
    import tgp_oracle as O
    from tgp.connect import DenseConnect
    for transposed in (False, True):
        raw = DenseConnect().dense_connect(adj=_to_dev(A, dev, transposed), s=S.to(dev)).cpu()
        torch.testing.assert_close(raw / scale, O.dense_connect(S, A) / scale, rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(_u(S, A, dev, transposed) / scale, torch.matmul(A, S) / scale, rtol=RTOL, atol=ATOL)
    if kind == "weighted":  # (negative weights make the degree normalisation of the post-processing ill-conditioned)
        _check(S, A, X, dev)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("B,N,Kc,F,p", [(32, 1024, 128, 64, 0.02), (32, 1000, 100, 64, 0.02), (16, 1000, 200, 64, 0.02),
                                        (16, 1000, 200, 64, 0.5), (4, 2048, 512, 128, 0.01), (4, 2048, 512, 128, 0.3)])
def test_layouts_and_tails(dev, transposed, B, N, Kc, F, p):
    S, X, g = _inputs(B, N, Kc, F, seed=N + Kc)
    A = _adj(B, N, p, g)
    A.diagonal(dim1=1, dim2=2).zero_()
    _check(S, A, X, dev, transposed)


@pytest.mark.parametrize("bad", ["inf", "nan", "-inf"])
@pytest.mark.parametrize("transposed", [False, True])
def test_non_finite_s(dev, bad, transposed):
    """0 * Inf = NaN: a chunk whose S rows hold an Inf or NaN is multiplied in full, so U = A S has the NaN / Inf
    pattern of torch.matmul."""
    B, N, Kc = B32, 1024, 128
    S, _, g = _inputs(B, N, Kc, 4, seed=10)
    v = float(bad)
    S[0, 37, 5] = v
    S[1, 700, 127] = v
    S[1, 1023, 0] = v
    A = _adj(B, N, 0.02, g)
    got = _u(S, A, dev, transposed)
    want = torch.matmul(A, S)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and torch.equal(got[torch.isinf(got)], want[torch.isinf(want)])
    torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL, equal_nan=True)
    from tgp.connect import DenseConnect
    raw = DenseConnect().dense_connect(adj=_to_dev(A, dev, transposed), s=S.to(dev)).cpu()
    ref = torch.matmul(S.transpose(1, 2), want)  # the kernels' association: S^T (A S)
    assert torch.equal(torch.isnan(raw), torch.isnan(ref))
    torch.testing.assert_close(raw, ref, rtol=RTOL, atol=ATOL, equal_nan=True)


def test_nan_and_inf_in_a_are_kept(dev):
    B, N, Kc = B32, 1024, 128
    S, _, g = _inputs(B, N, Kc, 4, seed=11)
    A = _adj(B, N, 0.02, g)
    A[0, 3, 900] = float("nan")
    A[1, 600, 2] = float("inf")
    A[1, 601, 2] = float("-inf")
    got = _u(S, A, dev)
    want = torch.matmul(A, S)
    assert torch.isnan(got[0, 3]).all() and torch.equal(torch.isnan(got), torch.isnan(want))
    torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL, equal_nan=True)


@pytest.mark.parametrize("p", [0.02, 0.3])
def test_deterministic(dev, p):
    from tgp.connect import DenseConnect
    S, X, g = _inputs(B32, 1024, 128, 64, seed=12)
    A = _adj(B32, 1024, p, g).to(dev)
    conn = DenseConnect()
    r1 = conn.dense_connect(adj=A, s=S.to(dev))
    r2 = conn.dense_connect(adj=A, s=S.to(dev))
    assert torch.equal(r1, r2)
    assert torch.equal(_u(S, A.cpu(), dev), _u(S, A.cpu(), dev))


def test_training_forward_at_c2_shape(dev):
    """U from tgp_dense_pool_train_fwd_f32 at the headline shape (32 graphs, N = 1024, K = 128), bench-like A."""
    B, N, Kc = 32, 1024, 128
    S, _, g = _inputs(B, N, Kc, 4, seed=13)
    A = _adj(B, N, 0.01, g)
    A.diagonal(dim1=1, dim2=2).zero_()
    got = _u(S, A, dev)
    torch.testing.assert_close(got, torch.matmul(A, S), rtol=RTOL, atol=ATOL)
