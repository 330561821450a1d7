"""The wide sparse front-end of U = A S (gemm_mfma.h, MODE 3 / MODE 4 with a row-major A): 128-column chunks of A walked
from the registers that loaded them, in front of the 32-column stages of tests/test_gpu_sparse_walk.py.  What can go wrong
here is a wide chunk that is dropped, taken twice, walked against the wrong one of the two LDS buffers of S rows or from
the wrong register set, a hand-over to the 32-column loop at the wrong k, and a chunk that is walked although it should
have been multiplied (an Inf in its S rows).

As in test_gpu_sparse_walk.py every graph of a batch is its own problem, so one call per shape carries all the patterns.
With a one-hot S and A in {0, 1} the raw S^T A S is a matrix of small integers, compared for equality with the integer
computation on the host; the same patterns with softmax S and real weights, plus the special values, are compared with
float64 at the project's fp32 bar.

Reference: dense_conn.py:111-122, base_reduce.py:158-161."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-5  # the reference's own fp32 tolerance
K, F, BK, WIDE = 128, 16, 32, 128
WIDE_GROUPS = 896   # TGP_SPARSE_WIDE_GROUPS: a 128 x 128 chunk with more groups of 4 holding a nonzero is handed over
# (B, N): the smallest batches that pass the 256-tile gate
SHAPES = [(256, 96),   # no wide chunk: the front-end runs zero times
          (256, 128),  # exactly one wide chunk, the 32-column loop runs zero stages
          (128, 160),  # one wide chunk, then one 32-column stage; the second row tile is partial
          (128, 256),  # two wide chunks
          (86, 384),   # three: an odd count, both buffer parities
          (64, 544)]   # four wide chunks and a 32-column tail
IDS = [f"B{b}-N{n}" for b, n in SHAPES]
SPECIALS = ("inf_in_s", "nan_in_a", "inf_in_a")


def _positions(N):
    """First, middle and last wide-chunk position (none at N < 128)."""
    w = N // WIDE
    return sorted({0, w // 2, w - 1}) if w else []


def _plan(B, N):
    """(pattern, argument, special, special position) per graph: the patterns once, then a 2 % graph per special value
    and position (and one whose zeros are all -0.0), then the patterns again until the batch is full."""
    w = N // WIDE
    pats = [("zeros", None), ("sparse", None), ("dense_row", None)]
    pats += [("wide", c) for c in range(w)]            # a fully dense 128-column block: the hand-over at c, 2 % after it
    pats += [("dense32", s) for s in range(N // BK)]   # a fully dense 32-column block at every 32-column position
    pats += [(f"block{wd}", c) for wd in (8, 16) for c in range(w)]  # stay under WIDE_GROUPS: walked
    plan = [(n, a, None, None) for n, a in pats]
    plan += [("sparse", None, sp, c) for sp in SPECIALS for c in (_positions(N) or [None])]
    plan += [("sparse", None, "neg_zero", None)]
    assert len(plan) <= B, (len(plan), B)
    return plan + [plan[i % len(pats)] for i in range(B - len(plan))]


def _groups(chunk):
    """Groups of 4 consecutive values of a [rows][128] chunk that hold a nonzero."""
    return int((chunk.reshape(chunk.size(0), -1, 4) != 0).any(-1).sum())


@functools.lru_cache(maxsize=None)
def _binary_batch(B, N):
    """0/1 adjacencies (about 2 % nonzeros, symmetric, then the pattern's blocks), one-hot S, small-integer X."""
    g = torch.Generator().manual_seed(3000 * B + N)
    A = (torch.rand(B, N, N, generator=g) < 0.01).float()
    A = torch.maximum(A, A.transpose(1, 2))
    for b, (name, arg, _, _) in enumerate(_plan(B, N)):
        if name == "zeros":
            A[b].zero_()
        elif name == "dense_row":   # one wave walks ~128 nonzeros per chunk, the others ~3
            A[b, (7 * b + 3) % N, :] = 1.0
        elif name == "wide":
            A[b, :, WIDE * arg:WIDE * (arg + 1)] = 1.0
            assert _groups(A[b, :128, WIDE * arg:WIDE * (arg + 1)]) > WIDE_GROUPS
        elif name == "dense32":
            A[b, :, BK * arg:BK * (arg + 1)] = 1.0
            if BK * arg < WIDE * (N // WIDE):
                c = BK * arg // WIDE
                assert _groups(A[b, :128, WIDE * c:WIDE * (c + 1)]) > WIDE_GROUPS
        elif name in ("block8", "block16"):
            wd = int(name[5:])
            c0 = WIDE * arg + (20 if wd == 8 else 64)
            A[b, :, c0:c0 + wd] = 1.0
            assert _groups(A[b, :128, WIDE * arg:WIDE * (arg + 1)]) <= WIDE_GROUPS
    assign = torch.randint(0, K, (B, N), generator=g)
    S = torch.nn.functional.one_hot(assign, K).float()
    X = torch.randint(-3, 4, (B, N, F), generator=g).float()
    return S, A, X


def _int_reference(S, A, X):
    S64 = S.double()
    raw = torch.bmm(S64.transpose(1, 2), torch.bmm(A.double(), S64))
    xp = torch.bmm(S64.transpose(1, 2), X.double())
    assert torch.equal(raw, raw.round()) and torch.equal(xp, xp.round()) and raw.abs().max() < 2 ** 24
    return raw.long(), xp.long()


@functools.lru_cache(maxsize=None)
def _binary_reference(B, N):
    """int64 S^T A S and S^T X (float64 products of small integers are exact; checked to be whole numbers below 2^24)."""
    return _int_reference(*_binary_batch(B, N))


@functools.lru_cache(maxsize=None)
def _weighted_batch(B, N):
    """The same patterns with real weights in A and a softmax S, plus the special values, each in a 2 % graph of its own
    and inside the first, a middle and the last wide chunk: an Inf in a row of S, a NaN in A, an Inf in A; and one graph
    whose zeros are all -0.0."""
    g = torch.Generator().manual_seed(4000 * B + N)
    _, A01, _ = _binary_batch(B, N)
    A = A01 * (torch.rand(B, N, N, generator=g) + 0.1)
    S = torch.softmax(torch.randn(B, N, K, generator=g), -1)
    X = torch.randn(B, N, F, generator=g)
    for b, (_, _, special, c) in enumerate(_plan(B, N)):
        col = N // 2 if c is None else WIDE * c
        if special == "inf_in_s":      # that chunk is handed over and takes the MFMAs: 0 * Inf = NaN as in torch
            S[b, col + 37, 7] = float("inf")
        elif special == "nan_in_a":
            A[b, 5, col + 29] = float("nan")
        elif special == "inf_in_a":
            A[b, N - 1, col + 1] = float("inf")
        elif special == "neg_zero":
            A[b][A[b] == 0] = -0.0
    return S, A, X


def _run(S, A, X, dev):
    """The kernels wrapper of tgp_dense_pool_f32 (what DenseSRCPooling.reduce_connect(..., want_raw=True) calls)."""
    from tgp import kernels
    x_pool, raw, _ = kernels.dense_pool(S.to(dev), A.to(dev), X.to(dev), want_raw=True, want_post=False)
    torch.cuda.synchronize()
    return x_pool.cpu(), raw.cpu()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def binary_outputs(dev):
    """The outputs for the 0/1 batch of every shape (computed once, shared by the tests below)."""
    return {shape: _run(*_binary_batch(*shape), dev) for shape in SHAPES}


def _names(B, N):
    return [f"{n}@{a}" if a is not None else n for n, a, _, _ in _plan(B, N)]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_binary_patterns_are_exact(binary_outputs, shape):
    """Raw S^T A S and S^T X of the 0/1 batch equal the int64 computation on the host, graph by graph."""
    x_pool, raw = binary_outputs[shape]
    raw_ref, xp_ref = _binary_reference(*shape)
    assert torch.equal(raw, raw.round()) and torch.equal(x_pool, x_pool.round())
    bad = [(b, n) for b, n in enumerate(_names(*shape)) if not torch.equal(raw[b].long(), raw_ref[b])]
    assert not bad, f"raw S^T A S differs from the integer reference in graphs {bad[:8]} ({len(bad)} in all)"
    assert torch.equal(x_pool.long(), xp_ref)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_binary_patterns_are_deterministic(dev, binary_outputs, shape):
    x_pool, raw = binary_outputs[shape]
    x_again, raw_again = _run(*_binary_batch(*shape), dev)
    assert torch.equal(raw.view(torch.int32), raw_again.view(torch.int32))
    assert torch.equal(x_pool.view(torch.int32), x_again.view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_weighted_patterns_and_special_values(dev, shape):
    """Softmax S, real weights, -0.0, NaN / Inf in A and Inf in S against float64 (the kernels' association S^T (A S)):
    NaNs and infinities in the same places, everything else at the fp32 bar."""
    S, A, X = _weighted_batch(*shape)
    x_pool, raw = _run(S, A, X, dev)
    S64 = S.double()
    raw_ref = torch.bmm(S64.transpose(1, 2), torch.bmm(A.double(), S64))
    xp_ref = torch.bmm(S64.transpose(1, 2), X.double())
    for b, (_, _, special, _) in enumerate(_plan(*shape)):  # the specials reach the output, and only they
        if special in ("inf_in_s", "nan_in_a"):
            assert torch.isnan(raw_ref[b]).any()
        elif special == "inf_in_a":
            assert torch.isinf(raw_ref[b]).any()
        else:
            assert torch.isfinite(raw_ref[b]).all()
    for got, ref in ((raw, raw_ref), (x_pool, xp_ref)):
        assert torch.equal(torch.isnan(got), torch.isnan(ref))
        assert torch.equal(torch.isinf(got), torch.isinf(ref))
        torch.testing.assert_close(got.double(), ref, rtol=RTOL, atol=ATOL, equal_nan=True)


def test_each_wide_chunk_meets_its_own_rows_of_s(dev, binary_outputs):
    """The panel order at two wide chunks: with the left or the right 128 columns of every A cleared, the remaining
    chunk alone gives the integer reference of that half (chunk 1 walked against chunk 0's S rows, or from chunk 0's
    registers, would give the other half's sums: the one-hot S assigns the two halves' nodes differently), and the two
    halves add up to the whole, exactly."""
    shape = (128, 256)
    S, A, X = _binary_batch(*shape)
    _, raw = binary_outputs[shape]
    halves = []
    for lo in (0, WIDE):
        Ah = A.clone()
        Ah[:, :, WIDE - lo:2 * WIDE - lo] = 0.0   # keeps columns lo .. lo + 127
        _, raw_h = _run(S, Ah, X, dev)
        ref_h, _ = _int_reference(S, Ah, X)
        assert torch.equal(raw_h.long(), ref_h)
        halves.append(raw_h)
    assert not torch.equal(halves[0], halves[1])
    assert torch.equal(halves[0] + halves[1], raw)
