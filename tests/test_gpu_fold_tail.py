"""The folded tail of the dense poolers' two-launch route (gemm_mfma.h, MODE 4) on the paths that reach it differently.

A workgroup gets to the tail either straight from the wide front-end, having walked the chunk that ends its k-range, or
from the 32-column stages.  It holds U either in the walk's sums alone (no MFMA ran: the sums go to the LDS operand
directly) or in the accumulators and the sums (the accumulators go first, the sums are added there).  The tail then
multiplies in two phases: S^T U, whose blocks are parked in the LDS words U_r occupied and stored while S^T X runs, the
column sums taken from the accumulators lane to lane.  What can go wrong: a row of U beyond N that is not a zero on the
direct path, a lost -0.0 / NaN / Inf, a wave that parks into U_r while another still reads it, a block of 16 x 16 given to
two waves or to none under K < 128 or F < 64, a column sum that misses a row or takes the diagonal.

Entry and checks as in test_gpu_dense_fold.py: one-hot S with 0/1 A and small-integer X for equality with the integer
result computed on the host; softmax S with weighted A against float64 at the project's fp32 bar, through the degree-
normalised output (so the column sums count), with self-loop removal on and off.  Every graph of a batch carries one
pattern, so one call per shape covers them all; every call is made twice and must repeat itself bit for bit.
Reference: dense_conn.py:111-122, base_reduce.py:158-161, utils/ops.py:282-335."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-5  # the reference's own fp32 tolerance
WIDE, BK = 128, 32
# (B, N): the smallest batches that pass the gate of 256 row tiles
SHAPES = [(256, 96),    # no front-end
          (256, 128),   # one wide chunk: the first wide stage is also the last, and the k-loop runs no stage
          (128, 160),   # a wide chunk, then a 32-column stage; second tile partial
          (128, 256),   # the last wide stage on buffer parity 1
          (86, 384),    # ... on parity 0
          (32, 928)]    # eight tiles, the last one partial
KS, FS = (68, 100, 128), (0, 4, 16, 60, 64)  # (the post-processing kernel of the route needs K > 64)
SWEEP_SHAPE = (256, 128)
# every K x F at the smallest shape with a front-end; one or two pairs at the others, each K and each F at least once more
CASES = [SWEEP_SHAPE + (k, f) for k in KS for f in FS]
CASES += [(256, 96, 100, 60), (256, 96, 128, 0), (128, 160, 68, 4), (128, 160, 128, 64), (128, 256, 128, 16),
          (128, 256, 100, 64), (86, 384, 128, 60), (86, 384, 68, 0), (32, 928, 128, 64), (32, 928, 100, 4)]
PATTERNS = ("zeros", "sparse", "last_wide_dense", "first_wide_dense", "dense32_behind_walk", "inf_in_s", "nan_in_a", "neg_zero")


def _columns(name, N):
    """The fully dense column range of a pattern (None: none)."""
    nw = N // WIDE  # chunks the wide front-end can take
    if name == "last_wide_dense":   # the hand-over to the 32-column stages falls in the last wide stage
        return (WIDE * (nw - 1), WIDE * nw) if nw else (BK, 2 * BK)
    if name == "first_wide_dense":  # everything is multiplied from the first stage on: the walk's sums stay zero
        return (0, min(WIDE, N))
    if name == "dense32_behind_walk":  # the accumulators and the walk's sums both hold something
        return (N - BK, N)
    return None


@functools.lru_cache(maxsize=None)
def _adjacency(B, N):
    """0/1 adjacencies: ~2 % nonzeros (symmetric), then the pattern of graph b, PATTERNS[b % 8]."""
    g = torch.Generator().manual_seed(77 * B + N)
    A = (torch.rand(B, N, N, generator=g) < 0.01).float()
    A = torch.maximum(A, A.transpose(1, 2))
    for b in range(B):
        name = PATTERNS[b % len(PATTERNS)]
        if name == "zeros":
            A[b].zero_()
        cols = _columns(name, N)
        if cols:
            A[b, :, cols[0]:cols[1]] = 1.0
    return A


@functools.lru_cache(maxsize=None)
def _one_hot_s(B, N, K):
    g = torch.Generator().manual_seed(1000 * B + N + 7 * K)
    return torch.nn.functional.one_hot(torch.randint(0, K, (B, N), generator=g), K).float()


@functools.lru_cache(maxsize=None)
def _softmax_s(B, N, K):
    g = torch.Generator().manual_seed(3000 * B + N + 7 * K)
    S = torch.softmax(torch.randn(B, N, K, generator=g), -1)
    for b in range(B):
        if PATTERNS[b % len(PATTERNS)] == "inf_in_s":
            S[b, N - 5, 7] = float("inf")  # a row of the last chunk: 0 * Inf = NaN, so that chunk is multiplied in full
    return S


def _binary(B, N, K, F):
    """One-hot S and small-integer X (with the 0/1 A every sum is an integer below 2^24).  S does not depend on F."""
    g = torch.Generator().manual_seed(4000 * B + N + 7 * F)
    return _one_hot_s(B, N, K), (torch.randint(-3, 4, (B, N, F), generator=g).float() if F else None)


def _weighted(B, N, K, F):
    g = torch.Generator().manual_seed(5000 * B + N + 7 * F)
    return _softmax_s(B, N, K), (torch.randn(B, N, F, generator=g) if F else None)


@functools.lru_cache(maxsize=None)
def _weighted_a(B, N):
    """Real weights on the 0/1 adjacencies; one NaN in the nan_in_a graphs; every zero a -0.0 in the neg_zero graphs."""
    g = torch.Generator().manual_seed(2000 * B + N)
    A = _adjacency(B, N) * (torch.rand(B, N, N, generator=g) + 0.1)
    for b in range(B):
        name = PATTERNS[b % len(PATTERNS)]
        if name == "nan_in_a":
            A[b, 5, N - 3] = float("nan")
        if name == "neg_zero":
            A[b][A[b] == 0] = -0.0
    return A


@functools.lru_cache(maxsize=None)
def _u64(kind, B, N, K):
    """float64 U = A S of a batch (shared by the feature widths)."""
    if kind == "binary":
        return torch.bmm(_adjacency(B, N).double(), _one_hot_s(B, N, K).double())
    return torch.bmm(_weighted_a(B, N).double(), _softmax_s(B, N, K).double())


def _reference(kind, B, N, K, F):
    """float64 S^T (A S) and S^T X (the kernels' association)."""
    S, X = (_binary if kind == "binary" else _weighted)(B, N, K, F)
    St = S.double().transpose(1, 2)
    return torch.bmm(St, _u64(kind, B, N, K)), (torch.bmm(St, X.double()) if F else None)


def test_patterns_meet_the_thresholds():
    """(no GPU work) The patterns put each 128-column chunk on the side of the front-end's threshold they are meant for
    (gemm_mfma.h: a wide chunk is sparse up to 896 groups of four values that hold a nonzero)."""
    for B, N in SHAPES:
        A = _adjacency(B, N)
        for b in range(len(PATTERNS)):
            name = PATTERNS[b]
            for c in range(N // WIDE):
                groups = int((A[b, :128, WIDE * c:WIDE * (c + 1)].reshape(128, 32, 4) != 0).any(-1).sum())
                cols = _columns(name, N)
                dense = cols is not None and cols[0] < WIDE * (c + 1) and cols[1] > WIDE * c
                assert (groups > 896) == dense, (B, N, name, c, groups)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def device_a(dev):
    """The adjacencies of a shape on the device, uploaded once: {(kind, B, N): tensor}."""
    cache = {}

    def get(kind, B, N):
        if (kind, B, N) not in cache:
            if kind == "binary":
                A = _adjacency(B, N).clone()
                for b in range(B):
                    if PATTERNS[b % len(PATTERNS)] == "neg_zero":
                        A[b][A[b] == 0] = -0.0
            else:
                A = _weighted_a(B, N)
            cache[(kind, B, N)] = A.to(dev)
        return cache[(kind, B, N)]
    return get


def _call_twice(s, a, x, flags, want_raw, want_post):
    """One call, made twice: the outputs on the host, having repeated themselves bit for bit."""
    from tgp import kernels
    outs = []
    for _ in range(2):
        out = kernels.dense_pool(s, a, x, flags, want_raw=want_raw, want_post=want_post)
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


def _ids(case):
    return "B{}-N{}-K{}-F{}".format(*case)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_binary_is_exact(dev, device_a, case):
    """Raw S^T A S and S^T X of the 0/1 batch equal the integer computation on the host, graph by graph."""
    B, N, K, F = case
    S, X = _binary(*case)
    x_pool, raw, _ = _call_twice(S.to(dev), device_a("binary", B, N), None if X is None else X.to(dev), 0, True, False)
    raw_ref, xp_ref = _reference("binary", *case)
    assert torch.equal(raw_ref, raw_ref.round()) and raw_ref.max() < 2 ** 24
    bad = [(b, PATTERNS[b % len(PATTERNS)]) for b in range(B) if not torch.equal(raw[b].long(), raw_ref[b].long())]
    assert not bad, f"raw S^T A S differs from the integer reference in graphs {bad[:8]} ({len(bad)} in all)"
    assert torch.equal(raw, raw.round())
    if F:
        assert torch.equal(xp_ref, xp_ref.round()) and torch.equal(x_pool.long(), xp_ref.long()) and torch.equal(x_pool, x_pool.round())
    else:
        assert x_pool is None


@pytest.mark.parametrize("rsl", [False, True], ids=["keep-loops", "remove-loops"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_weighted_against_float64(dev, device_a, case, rsl):
    """Softmax S, weighted A, -0.0, a NaN in A and an Inf in S against float64: NaNs and infinities in the same places,
    everything else at the fp32 bar; the degree-normalised adj_pool against the oracle's post-processing of the float64
    product, so the tail's column sums are part of the check."""
    import tgp_oracle as O
    from tgp import kernels
    B, N, K, F = case
    S, X = _weighted(*case)
    flags = kernels.dense_flags(rsl, True, True, False)
    x_pool, raw, adj_pool = _call_twice(S.to(dev), device_a("weighted", B, N), None if X is None else X.to(dev), flags, True, True)
    raw_ref, xp_ref = _reference("weighted", *case)
    by_name = {PATTERNS[b]: b for b in range(len(PATTERNS))}
    assert torch.isnan(raw_ref[by_name["inf_in_s"]]).any() and torch.isnan(raw_ref[by_name["nan_in_a"]]).any()
    assert all(torch.isfinite(raw_ref[by_name[n]]).all() for n in PATTERNS if n not in ("inf_in_s", "nan_in_a"))
    _check_against_f64(raw, raw_ref)
    if F:
        _check_against_f64(x_pool, xp_ref)
    else:
        assert x_pool is None
    _check_against_f64(adj_pool, O.postprocess_dense(raw_ref, rsl, True, True, False))


@pytest.mark.parametrize("shape", SHAPES, ids=[f"B{b}-N{n}" for b, n in SHAPES])
def test_shapes_take_the_folded_route(dev, device_a, shape):
    """Two device kernels per call: the checks above ran the tail, not the three launches."""
    from torch.profiler import ProfilerActivity, profile
    from tgp import kernels
    S, X = _binary(*shape, 68, 4)
    s, a, x = S.to(dev), device_a("binary", *shape), X.to(dev)
    kernels.dense_pool(s, a, x)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        kernels.dense_pool(s, a, x)
        torch.cuda.synchronize()
    assert sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA) == 2
