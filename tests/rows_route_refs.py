"""Plain-torch references, case data and the error norm of tests/test_gpu_rows_route_ops.py (the operators of the dense
poolers' un-padded rows route against float64).  Nothing here touches the GPU or the native library: the references
take a dtype and run in it, so the same code is the float64 reference and, in float32, ``e_oracle32``.
tests/test_rows_route_refs.py pins these helpers against the oracle and checks every committed case's conditioning."""
import itertools
import math

import torch

import tgp_oracle as O
from test_gpu_grad_paths import CAP, FACTOR, FLOOR


# ------------------------------------------------------------------------------------------------------- error norm
def graph_errors(got, ref, blocks=None):
    """[max|got - ref| / max|ref| per block]: ``blocks`` = (start, end) row ranges of a 2-D result, None = the leading
    dimension of a [B, ...] result.  A block whose reference is exactly zero gives 0.0 when ``got`` is exactly zero there
    and inf otherwise (it must come out exactly zero); an empty block gives 0.0."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    pairs = [(got[b], ref[b]) for b in range(ref.size(0))] if blocks is None else [(got[a:e], ref[a:e]) for a, e in blocks]
    errs = []
    for g, r in pairs:
        if r.numel() == 0:
            errs.append(0.0)
            continue
        scale = float(r.abs().max())
        if scale == 0.0:
            errs.append(0.0 if torch.equal(g, torch.zeros_like(g)) else math.inf)
        elif not bool(torch.isfinite(g).all()):
            errs.append(math.inf)
        else:
            errs.append(float((g - r).abs().max()) / scale)
    return errs


def bound_of(e32):
    return max(FACTOR * e32, FLOOR)


class Worst:
    """Collects (what, e_kernel, e_oracle32) per graph and output; one log line and the assertions per case."""

    def __init__(self, case):
        self.case, self.rows, self.fails = case, [], []

    def add(self, what, got, ref64, ref32, blocks=None):
        ek, e32 = graph_errors(got, ref64, blocks), graph_errors(ref32, ref64, blocks)
        for b, (k, o) in enumerate(zip(ek, e32)):
            bound = bound_of(o)
            self.rows.append((k / bound, k, o, bound, f"{what}[graph {b}]"))
            if bound > CAP:
                self.fails.append(f"{self.case}: {what}[graph {b}]: bound {bound:.3e} above {CAP:g} (e_oracle32 {o:.3e}): "
                                  f"ill-conditioned data")
            elif not k <= bound:
                self.fails.append(f"{self.case}: {what}[graph {b}]: e_kernel {k:.3e} above the bound {bound:.3e} "
                                  f"(e_oracle32 {o:.3e})")

    def fail(self, msg):
        self.fails.append(f"{self.case}: {msg}")

    def line(self):
        if not self.rows:
            return f"{self.case} | nothing compared"
        _, k, o, bound, what = max(self.rows, key=lambda r: r[0])
        ratio = max((r[1] / r[2] for r in self.rows if r[2] > 0), default=float("nan"))
        return (f"{self.case} | worst {what} | e_kernel {k:.2e} | e_oracle32 {o:.2e} | bound {bound:.2e} | "
                f"largest e_kernel/e_oracle32 {ratio:.3g}")

    def finish(self):
        print(self.line())
        assert not self.fails, "\n".join(self.fails[:40])


def ptr_of(sizes):
    return torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.long)


def blocks_of(sizes):
    p = ptr_of(sizes).tolist()
    return list(zip(p[:-1], p[1:]))


def batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))


# ----------------------------------------------------------------------- 1. S^T [Y0 | Y1 | Y2] and the post-processing
# name, graph sizes, K, F: what the case reaches in tgp_segment_gemm_tn3_post_f32 (csrc/dense.hip, csrc/dense_post.h).
# The node-range split counts are what segment3_splits gives for three right-hand sides.
TN3_CASES = [
    ("tiny", [40, 25, 33], 8, 16),                      # post_tiny_kernel; 1 split
    ("many_small", [1 + (7 * i) % 40 for i in range(300)], 16, 8),  # 1 split (900 workgroups already); one-node graphs
    ("k64", [130, 97, 160], 64, 24),                    # post_small_kernel at its upper edge; 2 splits
    ("lds_no_fold", [300, 5, 0, 130], 68, 70),          # post_lds_kernel, K % 16 != 0: transposing combine + re-read of
                                                        # raw; X width > 64, not a multiple of 4; an empty graph and one
                                                        # shorter than a split's node range; 3 splits
    ("lds_fold", [700, 90], 80, 33),                    # the transposing slab sum inside post_lds_kernel; 6 splits
                                                        # (remainders of both unrolled slab loops)
    ("lds_max", [1100], 176, 200),                      # POST_LDS_MAX_K, K F = 35200 > 8 blocks x 4096; 9 splits
    ("past_lds", [600, 450], 180, 12),                  # post_combine_kernel<4> + degree / scale / max-norm; 5 splits
    ("k_mod4", [260, 199], 70, 10),                     # post_combine_kernel<1> (K % 4 != 0); 3 splits
    ("wide_k", [400, 380], 260, 64),                    # K > 256: five 64-row tiles per product; 4 splits
    ("one_long", [3000], 72, 16),                       # 24 splits
]
FEWER_RHS_CASES = ("tiny", "lds_fold", "past_lds")      # also run with one and with two right-hand sides

# (remove_self_loops, degree_norm, adj_transpose = sums over dim -2, edge_weight_norm), as oracle.postprocess_dense and
# kernels.dense_flags take them; None = the plain product without post-processing
POST_FLAGS = [
    None,
    (False, False, False, False),
    (True, True, True, False),    # the batched default: self loops removed, degree norm with column sums
    (True, True, False, False),   # the same with row sums
    (True, True, True, True),     # the batched default + edge-weight norm
    (False, False, False, True),  # edge-weight norm alone
]


def tn3_inputs(sizes, k, f, seed):
    """float32 host data: S = softmax of random logits, X, and a weighted DIRECTED coalesced row-sorted list of about six
    entries per row without self loops (raw != raw^T, so a missed transpose shows)."""
    g = torch.Generator().manual_seed(seed)
    eis, off = [], 0
    for n in sizes:
        if n > 1:
            a = torch.rand(n, n, generator=g) < min(6.0 / n, 0.5)
            a.fill_diagonal_(False)
            eis.append(a.nonzero().t() + off)
        off += n
    ei = torch.cat(eis, 1) if eis else torch.zeros(2, 0, dtype=torch.long)
    ew = torch.rand(ei.size(1), generator=g) + 0.25
    n = sum(sizes)
    s = torch.softmax(2.0 * torch.randn(n, k, generator=g), -1)
    x = torch.randn(n, f, generator=g)
    return s, x, ei.contiguous(), ew


def tn3_case(name):
    """(sizes, K, F, S, X, edge_index, edge_weight) of a named case: the data both test modules use."""
    i = [c[0] for c in TN3_CASES].index(name)
    _, sizes, k, f = TN3_CASES[i]
    return (sizes, k, f) + tn3_inputs(sizes, k, f, seed=11 + i)


def spmm_ref(ei, ew, s):
    """T = A S in s.dtype on the host (what kernels.spmm_csr computes on the GPU)."""
    return torch.zeros_like(s).index_add_(0, ei[0], s[ei[1]] * ew.to(s.dtype)[:, None])


def seg_tn_ref(s, y, sizes):
    """[S_b^T Y_b for b]: a per-graph loop in the operands' dtype."""
    out = s.new_zeros(len(sizes), s.size(1), y.size(1))
    for b, (a, e) in enumerate(blocks_of(sizes)):
        if e > a:
            out[b] = s[a:e].t() @ y[a:e]
    return out


def post_ref(raw, flags, transpose0):
    """adj_pool of ``raw`` (or of its transpose) through oracle.postprocess_dense, in raw's dtype."""
    m = raw.transpose(1, 2) if transpose0 else raw
    return O.postprocess_dense(m, *flags)


# ---------------------------------------------------------------------------------- 2. products on column-block views
VIEW_KF = [(8, 6), (10, 7), (40, 24), (66, 10), (72, 16), (130, 33)]  # 1st, 2nd, 4th: blocks off the 16-byte grid
VIEW_SIZES = [150, 1, 0, 97, 64, 33]  # a graph of exactly one 64-row tile, one of a single row, an empty one
BIG = 1e30                            # what every element around the operands holds: a leaked load or store shows
SLAB_COUNTS = [1, 7, 8, 9, 40]        # slab_sum_split folds eight lanes per element


def view_layout(k, f, pad=4):
    """Column offsets of [T | X | 1 0 0 0 | S | T'] and the row stride, as functions._PoolUnbatchedFn.backward lays it out."""
    return dict(t=0, x=k, one=k + f, s=k + f + pad, v=2 * k + f + pad, ld=3 * k + f + pad)


def view_blocks(k, f, n, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(t=torch.randn(n, k, generator=g), x=torch.randn(n, f, generator=g),
                s=torch.softmax(torch.randn(n, k, generator=g), -1), v=torch.randn(n, k, generator=g))


def view_case(k, f):
    """(blocks t / x / s / v, bm [B,K,K], bx [B,2K,F]) on VIEW_SIZES: the data both test modules use."""
    g = torch.Generator().manual_seed(200 + k)
    B = len(VIEW_SIZES)
    return (view_blocks(k, f, sum(VIEW_SIZES), seed=100 + k), torch.randn(B, k, k, generator=g),
            torch.randn(B, 2 * k, f, generator=g))


def bmm_case(G, M, Nc, Kd):
    g = torch.Generator().manual_seed(G * 1000 + M)
    return torch.randn(G, M, Kd, generator=g), torch.randn(G, Kd, Nc, generator=g), torch.randn(G, M, Nc, generator=g)


def seg_nn_ref(a, bm, sizes):
    """out[rows of b] = a[rows of b] @ bm[b]."""
    out = a.new_zeros(a.size(0), bm.size(2))
    for b, (lo, hi) in enumerate(blocks_of(sizes)):
        if hi > lo:
            out[lo:hi] = a[lo:hi] @ bm[b]
    return out


def slab_ptr(rows, slabs):
    """Row ranges of ~equal length, as functions._slab_ptr cuts them."""
    return (torch.arange(slabs + 1, dtype=torch.long) * rows) // slabs


BMM_SHAPES = [(3, 45, 37, 70), (2, 65, 33, 31), (1, 130, 67, 97)]  # G, M, N, Kd: no multiple of 32 or 64


# ------------------------------------------------------------------------------------------------ 3. softmax_bwd_ex
SOFTMAX_K = [1, 3, 16, 17, 64, 65, 300]
SOFTMAX_FORMS = {  # name -> (graph sizes, padded rows per graph or None)
    "padded": ([13, 13, 13], 13),   # [B,N,K]: the graph of a row is row // N; 39 rows
    "batch": ([13, 1, 0, 21, 8], None),  # [Ntot,K] with a batch vector; 43 rows
    "one_graph": ([27], None),      # [Ntot,K] without one
}
SOFTMAX_TERMS = [c for r in range(4) for c in itertools.combinations(("extra", "mincut", "entropy"), r)]
ENT_SCALE = 1.3


def softmax_inputs(sizes, k, seed):
    """float32 host data; row 2 of S is all zero (a padded node)."""
    g = torch.Generator().manual_seed(seed)
    n = sum(sizes)
    s = torch.softmax(2.0 * torch.randn(n, k, generator=g), -1)
    s[2] = 0.0
    return dict(s=s, ds=torch.randn(n, k, generator=g), extra=torch.randn(n, k, generator=g),
                c1=torch.randn(len(sizes), generator=g), deg=4.0 * torch.rand(n, generator=g) + 0.5,
                ent_g=torch.tensor(0.7))


def softmax_case(form, k):
    sizes, _ = SOFTMAX_FORMS[form]
    return softmax_inputs(sizes, k, seed=300 + k + 1000 * list(SOFTMAX_FORMS).index(form))


def softmax_effective(s, ds, extra, c1, deg, ent_g, ent_scale, eps, graph):
    """g = ds + extra + 2 c1[graph] deg[row] S - ent_g ent_scale (log(S + eps) + S / (S + eps)); absent terms are None."""
    g = ds
    if extra is not None:
        g = g + extra
    if c1 is not None:
        g = g + 2.0 * (c1[graph] * deg).unsqueeze(-1) * s
    if ent_g is not None:
        g = g - ent_g * ent_scale * (torch.log(s + eps) + s / (s + eps))
    return g


def softmax_bwd_ex_ref(s, ds, extra, c1, deg, ent_g, ent_scale, eps, graph):
    """dy = S (g - sum_k g S) in the operands' dtype; s [rows,K], graph [rows] (int64)."""
    g = softmax_effective(s, ds, extra, c1, deg, ent_g, ent_scale, eps, graph)
    return s * (g - (g * s).sum(-1, keepdim=True))


def softmax_args(data, terms, dtype):
    """The optional operands a subset of terms selects, in ``dtype`` (None where the term is absent)."""
    c = lambda v: v.to(dtype)
    return dict(extra=c(data["extra"]) if "extra" in terms else None,
                c1=c(data["c1"]) if "mincut" in terms else None, deg=c(data["deg"]) if "mincut" in terms else None,
                ent_g=c(data["ent_g"]) if "entropy" in terms else None)
