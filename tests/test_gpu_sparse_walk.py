"""U = A S of the dense poolers' tiled path at the smallest shapes that take the zero-skipping kernel (gemm_mfma.h,
MODE 3), checked exactly.  What can go wrong in its k-loop is a chunk that is dropped, taken twice or walked from the wrong
stage buffer -- in a loop shorter than the two-deep pipeline's prologue, at an odd or even loop length, in the tail stages,
or at the switch to plain stages after two dense k-steps in a row.

Every graph of a batch is its own problem (one workgroup per graph and row tile), so one call per shape carries all the
patterns: graph b holds pattern b mod len(patterns).  With a one-hot S and A in {0, 1} the raw S^T A S is a matrix of
small integers and is compared for equality with the integer computation on the host: a wrong chunk is a wrong integer.
The same batch with softmax S and real weights, plus -0.0, NaN and Inf, is compared with float64 at the project's
fp32 bar.

The shapes are the smallest that engage the kernel: at least 256 tiles of 128 x 128, K = 128 (one column tile).
Reference: dense_conn.py:111-122, base_reduce.py:158-161."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-5  # the reference's own fp32 tolerance
K, F, BK = 128, 16, 32
# (B, N): nk = N / 32 k-steps
SHAPES = [(256, 96),   # nk = 3: tail stages only, partial row tile
          (256, 128),  # nk = 4: one steady pair of stages
          (128, 160),  # nk = 5: odd length, second row tile partial
          (86, 384),   # nk = 12: steady loop, 258 tiles (just over the gate)
          (64, 544)]   # nk = 17: long steady loop, odd length
IDS = [f"B{b}-N{n}" for b, n in SHAPES]


def _patterns(nk):
    """(name, dense k-steps) per graph: all zeros; 2 % alone; one dense 128 x 32 chunk at each position; alternating
    dense and sparse chunks (never two dense in a row: no switch to plain stages); two consecutive dense chunks from
    every s (the switch at either stage parity and next to the loop's end, 2 % chunks after it)."""
    pats = [("zeros", None), ("sparse", [])]
    pats += [(f"dense@{s}", [s]) for s in range(nk)]
    pats += [("alternating", list(range(0, nk, 2)))]
    pats += [(f"two@{s}", [s, s + 1]) for s in range(nk - 1)]
    return pats


@functools.lru_cache(maxsize=None)
def _binary_batch(B, N):
    """0/1 adjacencies (2 % random, symmetric, then the pattern's dense column blocks), one-hot S, small-integer X."""
    g = torch.Generator().manual_seed(1000 * B + N)
    pats = _patterns(N // BK)
    A = (torch.rand(B, N, N, generator=g) < 0.02).float()
    A = torch.maximum(A, A.transpose(1, 2))
    for b in range(B):
        name, dense = pats[b % len(pats)]
        if dense is None:
            A[b].zero_()
        else:
            for s in dense:
                A[b, :, BK * s:BK * (s + 1)] = 1.0
    assign = torch.randint(0, K, (B, N), generator=g)
    S = torch.nn.functional.one_hot(assign, K).float()
    X = torch.randint(-3, 4, (B, N, F), generator=g).float()
    return S, A, X


@functools.lru_cache(maxsize=None)
def _binary_reference(B, N):
    """int64 S^T A S and S^T X (float64 products of small integers are exact; checked to be whole numbers)."""
    S, A, X = _binary_batch(B, N)
    S64 = S.double()
    raw = torch.bmm(S64.transpose(1, 2), torch.bmm(A.double(), S64))
    xp = torch.bmm(S64.transpose(1, 2), X.double())
    assert torch.equal(raw, raw.round()) and torch.equal(xp, xp.round()) and raw.max() < 2 ** 24
    return raw.long(), xp.long()


# the special values go into graphs of the patterns' second round, one each: a 2 % graph, then dense@0, dense@1, dense@2
SPECIALS = ("inf_in_s", "neg_zero", "nan_in_a", "inf_in_a")


def _first_special(N):
    return len(_patterns(N // BK)) + 1


@functools.lru_cache(maxsize=None)
def _weighted_batch(B, N):
    """The same patterns with real weights in A and a softmax S, plus -0.0 entries, one NaN and one Inf in A, and one Inf
    in a row of S (each in a graph of its own)."""
    g = torch.Generator().manual_seed(2000 * B + N)
    _, A01, _ = _binary_batch(B, N)
    A = A01 * (torch.rand(B, N, N, generator=g) + 0.1)
    S = torch.softmax(torch.randn(B, N, K, generator=g), -1)
    X = torch.randn(B, N, F, generator=g)
    b = _first_special(N)
    assert b + len(SPECIALS) <= B
    S[b, N // 2, 7] = float("inf")               # (a 2 % graph) that chunk takes the MFMAs: 0 * Inf = NaN as in torch
    A[b + 1][A[b + 1] == 0] = -0.0               # every zero of the graph is a negative zero
    A[b + 2, 5, N - 3] = float("nan")
    A[b + 3, N - 1, 1] = float("inf")
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
    pats = _patterns(N // BK)
    return [pats[b % len(pats)][0] for b in range(B)]


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
    b = _first_special(shape[1])
    assert torch.isnan(raw_ref[b]).any() and torch.isnan(raw_ref[b + 2]).any()  # the specials reach the output
    assert torch.isinf(raw_ref[b + 3]).any() and torch.isfinite(raw_ref[:b]).all()
    assert torch.isfinite(raw_ref[b + 1]).all()
    for got, ref in ((raw, raw_ref), (x_pool, xp_ref)):
        assert torch.equal(torch.isnan(got), torch.isnan(ref))
        assert torch.equal(torch.isinf(got), torch.isinf(ref))
        torch.testing.assert_close(got.double(), ref, rtol=RTOL, atol=ATOL, equal_nan=True)
