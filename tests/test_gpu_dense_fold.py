"""The dense poolers' two-launch route: S^T [U | X] folded into the zero-skipping U = A S launch (gemm_mfma.h, MODE 4).

A workgroup of that launch ends its k-loop holding the complete rows U[128 r .. 128 r + 127, :] of its graph and
multiplies them, and the same rows of X, by S_r^T: one K x (K + F) partial per 128-row tile, added up by
post_rows_kernel.  What can go wrong is in that tail: a row of U or S beyond N that is not a zero, an operand value at the
wrong place of its swizzled LDS row, a 16 x 16 block given to two waves or to none, a partial output tile (K < 128, F < 64), the column
sums of the degree vector, and the gate that sends everything else down the three launches.

Inputs as in test_gpu_sparse_walk.py: every graph of a batch is its own problem and carries one pattern of dense and
sparse 128 x 32 chunks of A.  One-hot S with 0/1 A is compared for equality with the integer computation on the host;
softmax S with weighted A, -0.0, NaN and Inf with float64 at the project's fp32 bar.
Reference: dense_conn.py:111-122, base_reduce.py:158-161, utils/ops.py:282-335."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-5  # the reference's own fp32 tolerance
K, F, BK = 128, 16, 32
# (B, N) -> row tiles of 128 per graph.  At least 256 tiles and at most 8 per graph take the folded route.
SHAPES = [(256, 96),    # 1: partial tile, nk = 3
          (256, 100),   # 1: N no multiple of 32: zero-filled S rows inside the tail's operand
          (256, 128),   # 1
          (128, 160),   # 2: second tile partial
          (86, 384),    # 3: 258 tiles, just over the gate
          (32, 928),    # 8: the limit, last tile partial
          (29, 1056)]   # 9: over the limit -> the three launches
IDS = [f"B{b}-N{n}" for b, n in SHAPES]
SPECIALS = ("inf_in_s", "neg_zero", "nan_in_a", "inf_in_a")


def _folds(B, N, f=F, k=K):
    tiles = (N + 127) // 128
    return B * tiles >= 256 and tiles <= 8 and k <= 128 and f <= 64


def _patterns(B, N):
    """(name, dense k-steps) per graph: all zeros; 2 % alone; one dense chunk at each position; alternating; two dense in
    a row from each position.  Where the batch has fewer graphs than that (the long graphs), the positions are the first
    two, the middle one and the last two."""
    nk = (N + BK - 1) // BK
    pos = list(range(nk))
    if 2 * nk + 2 + len(SPECIALS) + 1 > B:
        pos = sorted({0, 1, nk // 2, nk - 2, nk - 1})
    pats = [("zeros", None), ("sparse", [])]
    pats += [(f"dense@{s}", [s]) for s in pos]
    pats += [("alternating", list(range(0, nk, 2)))]
    pats += [(f"two@{s}", [s, s + 1]) for s in pos if s + 1 < nk]
    assert len(pats) + 1 + len(SPECIALS) <= B
    return pats


@functools.lru_cache(maxsize=2)  # (the long graphs' adjacencies are > 100 MB each)
def _binary_batch(B, N, f=F, k=K):
    """0/1 adjacencies (2 % random, symmetric, then the pattern's dense column blocks), one-hot S, small-integer X."""
    g = torch.Generator().manual_seed(1000 * B + N + 7 * f + k)
    pats = _patterns(B, N)
    A = (torch.rand(B, N, N, generator=g) < 0.02).float()
    A = torch.maximum(A, A.transpose(1, 2))
    for b in range(B):
        _, dense = pats[b % len(pats)]
        if dense is None:
            A[b].zero_()
        else:
            for s in dense:
                A[b, :, BK * s:BK * (s + 1)] = 1.0
    assign = torch.randint(0, k, (B, N), generator=g)
    S = torch.nn.functional.one_hot(assign, k).float()
    X = torch.randint(-3, 4, (B, N, f), generator=g).float() if f else None
    return S, A, X


@functools.lru_cache(maxsize=2)
def _weighted_batch(B, N, f=F, k=K):
    """The same patterns with real weights in A and a softmax S, plus -0.0 entries, one NaN and one Inf in A, and one Inf
    in a row of S (each in a graph of its own, in the patterns' second round)."""
    g = torch.Generator().manual_seed(2000 * B + N + 7 * f + k)
    _, A01, _ = _binary_batch(B, N, f, k)
    A = A01 * (torch.rand(B, N, N, generator=g) + 0.1)
    S = torch.softmax(torch.randn(B, N, k, generator=g), -1)
    X = torch.randn(B, N, f, generator=g) if f else None
    b = len(_patterns(B, N)) + 1
    S[b, N // 2, 7] = float("inf")               # (a 2 % graph) that chunk takes the MFMAs: 0 * Inf = NaN as in torch
    A[b + 1][A[b + 1] == 0] = -0.0               # every zero of the graph is a negative zero
    A[b + 2, 5, N - 3] = float("nan")
    A[b + 3, N - 1, 1] = float("inf")
    return S, A, X


@functools.lru_cache(maxsize=None)
def _reference(kind, B, N, f=F, k=K):
    """float64 S^T (A S) and S^T X (the kernels' association) of a batch, computed once."""
    S, A, X = (_binary_batch if kind == "binary" else _weighted_batch)(B, N, f, k)
    S64 = S.double()
    raw = torch.bmm(S64.transpose(1, 2), torch.bmm(A.double(), S64))
    xp = torch.bmm(S64.transpose(1, 2), X.double()) if X is not None else None
    return raw, xp


def _kernels_of(fn):
    """Device kernels (and memsets) of one call, counted the way bench.py's count_kernels does."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def _run(S, A, X, dev, flags=0, want_raw=True, want_post=False, **kw):
    from tgp import kernels
    s, a, x = _to(dev, S, A, X)
    out = kernels.dense_pool(s, a, x, flags, want_raw=want_raw, want_post=want_post, **kw)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu() for t in out]


def _check_against_f64(got, ref):
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert torch.equal(torch.isinf(got), torch.isinf(ref))
    torch.testing.assert_close(got.double(), ref, rtol=RTOL, atol=ATOL, equal_nan=True)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def binary_outputs(dev):
    """The outputs for the 0/1 batch of every shape (computed once, shared by the tests below)."""
    return {shape: _run(*_binary_batch(*shape), dev) for shape in SHAPES}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_binary_patterns_are_exact(binary_outputs, shape):
    """Raw S^T A S and S^T X of the 0/1 batch equal the int64 computation on the host, graph by graph."""
    x_pool, raw, _ = binary_outputs[shape]
    raw_ref, xp_ref = _reference("binary", *shape)
    assert torch.equal(raw_ref, raw_ref.round()) and torch.equal(xp_ref, xp_ref.round()) and raw_ref.max() < 2 ** 24
    pats = _patterns(*shape)
    bad = [(b, pats[b % len(pats)][0]) for b in range(shape[0]) if not torch.equal(raw[b].long(), raw_ref[b].long())]
    assert not bad, f"raw S^T A S differs from the integer reference in graphs {bad[:8]} ({len(bad)} in all)"
    assert torch.equal(raw, raw.round()) and torch.equal(x_pool.long(), xp_ref.long()) and torch.equal(x_pool, x_pool.round())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_two_calls_are_bitwise_equal(dev, binary_outputs, shape):
    x_pool, raw, _ = binary_outputs[shape]
    x_again, raw_again, _ = _run(*_binary_batch(*shape), dev)
    assert torch.equal(raw.view(torch.int32), raw_again.view(torch.int32))
    assert torch.equal(x_pool.view(torch.int32), x_again.view(torch.int32))
    S, A, X = _weighted_batch(*shape)
    one, two = _run(S, A, X, dev, want_post=True), _run(S, A, X, dev, want_post=True)
    for u, v in zip(one, two):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_launch_count(dev, shape):
    """Two device kernels inside the gate, the three launches outside it."""
    from tgp import kernels
    s, a, x = _to(dev, *_binary_batch(*shape))
    n = _kernels_of(lambda: kernels.dense_pool(s, a, x, kernels.dense_flags(True, True, True, False)))
    assert n == (2 if _folds(*shape) else 3)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_weighted_patterns_and_special_values(dev, shape):
    """Softmax S, real weights, -0.0, NaN / Inf in A and Inf in S against float64: NaNs and infinities in the same places,
    everything else at the fp32 bar; adj_pool against the oracle's post-processing of the float64 product."""
    import tgp_oracle as O
    from tgp import kernels
    S, A, X = _weighted_batch(*shape)
    x_pool, raw, adj_pool = _run(S, A, X, dev, kernels.dense_flags(True, True, True, False), want_post=True)
    raw_ref, xp_ref = _reference("weighted", *shape)
    b = len(_patterns(*shape)) + 1
    assert torch.isnan(raw_ref[b]).any() and torch.isnan(raw_ref[b + 2]).any()  # the specials reach the output
    assert torch.isinf(raw_ref[b + 3]).any() and torch.isfinite(raw_ref[:b]).all() and torch.isfinite(raw_ref[b + 1]).all()
    _check_against_f64(raw, raw_ref)
    _check_against_f64(x_pool, xp_ref)
    _check_against_f64(adj_pool, O.postprocess_dense(raw_ref, True, True, True, False))


FOLD_SHAPE = (256, 128)


@pytest.mark.parametrize("f", [0, 16, 20, 64, 96], ids=lambda f: f"F{f}")
def test_feature_widths(dev, f):
    """X absent, F = 16, 20 (a partial 16-column block), 64 (the limit) fold; F = 96 takes the three launches."""
    from tgp import kernels
    S, A, X = _weighted_batch(*FOLD_SHAPE, f)
    x_pool, raw, _ = _run(S, A, X, dev)
    raw_ref, xp_ref = _reference("weighted", *FOLD_SHAPE, f)
    _check_against_f64(raw, raw_ref)
    if f:
        _check_against_f64(x_pool, xp_ref)
    else:
        assert x_pool is None
    s, a, x = _to(dev, S, A, X)
    assert _kernels_of(lambda: kernels.dense_pool(s, a, x)) == (2 if _folds(*FOLD_SHAPE, f) else 3)
    Sb, Ab, Xb = _binary_batch(*FOLD_SHAPE, f)
    xb, rb, _ = _run(Sb, Ab, Xb, dev)
    rb_ref, xb_ref = _reference("binary", *FOLD_SHAPE, f)
    assert torch.equal(rb.double(), rb_ref) and (not f or torch.equal(xb.double(), xb_ref))


def test_partial_output_tile(dev):
    """K = 100: the last 16 x 16 blocks of S^T U and the 32-column groups of U are partial."""
    from tgp import kernels
    k = 100
    S, A, X = _weighted_batch(*FOLD_SHAPE, F, k)
    x_pool, raw, adj_pool = _run(S, A, X, dev, kernels.dense_flags(True, True, True, False), want_post=True)
    raw_ref, xp_ref = _reference("weighted", *FOLD_SHAPE, F, k)
    import tgp_oracle as O
    _check_against_f64(raw, raw_ref)
    _check_against_f64(x_pool, xp_ref)
    _check_against_f64(adj_pool, O.postprocess_dense(raw_ref, True, True, True, False))
    s, a, x = _to(dev, S, A, X)
    assert _kernels_of(lambda: kernels.dense_pool(s, a, x)) == 2
    Sb, Ab, Xb = _binary_batch(*FOLD_SHAPE, F, k)
    xb, rb, _ = _run(Sb, Ab, Xb, dev)
    rb_ref, xb_ref = _reference("binary", *FOLD_SHAPE, F, k)
    assert torch.equal(rb.double(), rb_ref) and torch.equal(xb.double(), xb_ref)


FLAG_SHAPE = (128, 160)


@pytest.mark.parametrize("transposed", [False, True], ids=["A", "A^T-view"])
@pytest.mark.parametrize("rsl", [False, True], ids=["keep-loops", "remove-loops"])
@pytest.mark.parametrize("dn", [False, True], ids=["no-norm", "degree-norm"])
def test_flags_and_adjacency_layout(dev, transposed, rsl, dn):
    """remove_self_loops x degree_norm, with A contiguous and as the transposed view of a contiguous A^T (the k-major
    instantiation): the column sums the tail leaves are the degrees of the post-processing."""
    import tgp_oracle as O
    from tgp import kernels
    S, A, X = _weighted_batch(*FLAG_SHAPE)
    s, a, x = _to(dev, S, A, X)
    if transposed:
        a = a.transpose(1, 2).contiguous().transpose(1, 2)
        assert not a.is_contiguous()
    flags = kernels.dense_flags(rsl, dn, True, False)
    x_pool, raw, adj_pool = kernels.dense_pool(s, a, x, flags, want_raw=True, want_post=True)
    raw_ref, xp_ref = _reference("weighted", *FLAG_SHAPE)
    _check_against_f64(raw.cpu(), raw_ref)
    _check_against_f64(x_pool.cpu(), xp_ref)
    _check_against_f64(adj_pool.cpu(), O.postprocess_dense(raw_ref, rsl, dn, True, False))
    assert _kernels_of(lambda: kernels.dense_pool(s, a, x, flags)) == 2


def test_outputs_asked_for(dev):
    """want_raw without want_post, want_post without want_raw, both; out_x / out_adj given: the same values in each."""
    from tgp import kernels
    S, A, X = _weighted_batch(*FLAG_SHAPE)
    s, a, x = _to(dev, S, A, X)
    flags = kernels.dense_flags(True, True, True, False)
    x_both, raw_both, pool_both = kernels.dense_pool(s, a, x, flags, want_raw=True, want_post=True)
    x_raw, raw_only, none_pool = kernels.dense_pool(s, a, x, flags, want_raw=True, want_post=False)
    x_post, none_raw, pool_only = kernels.dense_pool(s, a, x, flags, want_raw=False, want_post=True)
    assert none_pool is None and none_raw is None
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    assert torch.equal(bits(raw_only), bits(raw_both)) and torch.equal(bits(pool_only), bits(pool_both))
    assert torch.equal(bits(x_raw), bits(x_both)) and torch.equal(bits(x_post), bits(x_both))
    B = FLAG_SHAPE[0]
    buf_x = torch.full((B + 1, K, F), float("nan"), device=dev)
    buf_a = torch.full((B + 1, K, K), float("nan"), device=dev)
    ox, _, oa = kernels.dense_pool(s, a, x, flags, out_x=buf_x[:B], out_adj=buf_a[:B])
    assert ox.data_ptr() == buf_x.data_ptr() and oa.data_ptr() == buf_a.data_ptr()
    assert torch.equal(bits(buf_x[:B]), bits(x_both)) and torch.equal(bits(buf_a[:B]), bits(pool_both))
    assert torch.isnan(buf_x[B]).all() and torch.isnan(buf_a[B]).all()  # nothing beyond the outputs was touched


def test_training_entry_keeps_three_launches(dev):
    """The training forward needs U in memory: it keeps U = A S, S^T [U | X] and the post-processing as three launches,
    and its raw product agrees with the folded route's at the fp32 bar."""
    from tgp import kernels
    S, A, X = _weighted_batch(*FOLD_SHAPE)
    b = len(_patterns(*FOLD_SHAPE)) + 1  # the graphs in front of the special values
    s, a, x = _to(dev, S[:b].repeat(FOLD_SHAPE[0] // b + 1, 1, 1)[:FOLD_SHAPE[0]],
                  A[:b].repeat(FOLD_SHAPE[0] // b + 1, 1, 1)[:FOLD_SHAPE[0]],
                  X[:b].repeat(FOLD_SHAPE[0] // b + 1, 1, 1)[:FOLD_SHAPE[0]])
    flags = kernels.dense_flags(True, True, True, False)
    acat = torch.empty(FOLD_SHAPE[0], FOLD_SHAPE[1], 3 * K + F + kernels.TRAIN_PAD, device=dev)
    assert _kernels_of(lambda: kernels.dense_pool_train_fwd(s, a, x, flags, acat, False)) == 3
    x_t, raw_t, pool_t, _ = kernels.dense_pool_train_fwd(s, a, x, flags, acat, False)
    x_f, raw_f, pool_f = kernels.dense_pool(s, a, x, flags, want_raw=True)
    torch.testing.assert_close(acat[:, :, :K], torch.bmm(a, s), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(raw_f, raw_t, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(x_f, x_t, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(pool_f, pool_t, rtol=RTOL, atol=ATOL)
