"""ASAPooling on the MI355X: the public class against the reference's stored results, each forward and backward kernel
alone against float64 with a bound derived from its arithmetic (never tuned), the arg-max positions exactly, run-to-run
determinism of results and gradients, gradients one upstream path at a time at fp32's own error (the helper of
test_gpu_grad_paths.py), the memory the native route may not take (nothing of size E x F), non-finite inputs against
the composed form, and which inputs take which route.  Without the feature this module fails at import."""
import os

import pytest
import torch

import asap_restatement as R
from test_gpu_grad_paths import check_grad_paths

from tgp import functions as Fn
from tgp import kernels as K
from tgp.leconv import LEConv
from tgp.poolers import ASAPooling
from tgp.utils import add_remaining_self_loops
from tgp.utils import ops as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_asap_v1.pt"), weights_only=True)["cases"]
GNNS = {None: None, "graphconv": None}  # filled below: the fixture's GNN case hands a class with edge weights
U = 2.0 ** -24  # fp32 unit roundoff


class GraphConvW(torch.nn.Module):
    """PyG's GraphConv with edge weights (the fixture's ``GNN=`` class): lin_rel(sum_j w_ji x_j) + lin_root(x_i)."""

    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__()
        self.lin_rel = torch.nn.Linear(in_channels, out_channels, bias=bias)
        self.lin_root = torch.nn.Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_rel.reset_parameters()
        self.lin_root.reset_parameters()

    def forward(self, x, edge_index, edge_weight=None):
        msg = x[edge_index[0]] if edge_weight is None else x[edge_index[0]] * edge_weight.view(-1, 1)
        return self.lin_rel(torch.zeros_like(x).index_add_(0, edge_index[1], msg)) + self.lin_root(x)


GNNS["graphconv"] = GraphConvW


def dev():
    return torch.device("cuda:0")


def build(c, requires_grad=False, dtype=torch.float32):
    p = ASAPooling(GNN=GNNS[c["gnn"]], **c["cfg"]).eval()
    p.load_state_dict(c["params"])
    p = p.to(dev(), dtype)
    for q in p.parameters():
        q.requires_grad_(requires_grad)
    return p


def forward(p, c, dtype=torch.float32, ew_grad=False):
    i = c["inputs"]
    d = dev()
    ew = None if i["edge_weight"] is None else i["edge_weight"].to(d, dtype).requires_grad_(ew_grad)
    return p(x=i["x"].to(d, dtype), adj=i["edge_index"].to(d), edge_weight=ew,
             batch=None if i["batch"] is None else i["batch"].to(d))


class Routes:
    """Counts the calls of the native attention while a block runs."""

    def __enter__(self):
        self.native, self._orig = 0, Fn.asap_attention

        def counted(*a, **k):
            self.native += 1
            return self._orig(*a, **k)

        Fn.asap_attention = counted
        return self

    def __exit__(self, *exc):
        Fn.asap_attention = self._orig


def check_output(out, e, name, tol=1e-5):
    so = out.so
    assert torch.equal(so.node_index.cpu(), e["so"]["node_index"]), name
    assert torch.equal(so.cluster_index.cpu(), e["so"]["cluster_index"]), name
    assert so.num_nodes == e["so"]["num_nodes"] and so.num_supernodes == e["so"]["num_supernodes"]
    assert torch.equal(out.edge_index.cpu(), e["edge_index"]), name
    assert torch.equal(out.batch.cpu(), e["batch"]), name
    torch.testing.assert_close(so.weight.detach().cpu().float(), e["so"]["weight"], rtol=tol, atol=tol)
    torch.testing.assert_close(out.x.detach().cpu().float(), e["x"], rtol=tol, atol=tol)
    if e["edge_weight"] is None:
        assert out.edge_weight is None
    else:
        torch.testing.assert_close(out.edge_weight.detach().cpu().float(), e["edge_weight"], rtol=tol, atol=tol)


# ------------------------------------------------------------------------------------------------ the public class
@pytest.mark.parametrize("grad", [False, True], ids=["no_grad", "grad"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_parity_through_the_public_class(name, grad):
    """The native kernels run (counted) with and without grad; under grad the attention and the score are one autograd
    node each."""
    c = CASES[name]
    p = build(c, requires_grad=grad)
    with Routes() as r, torch.set_grad_enabled(grad):
        out = forward(p, c)
    assert r.native == 1
    assert out.x.requires_grad == grad and out.so.weight.requires_grad == grad
    check_output(out, c["expected"], name)


@pytest.mark.parametrize("name", ["asap_weighted", "asap_gnn", "asap_one_column", "asap_duplicates"])
def test_the_fitness_pieces_match_the_fixture(name):
    c = CASES[name]
    p = build(c)
    i, e = c["inputs"], c["expected"]
    x = i["x"].to(dev())
    x = x.view(-1, 1) if x.dim() == 1 else x
    ew = None if i["edge_weight"] is None else i["edge_weight"].to(dev())
    ei, ew = add_remaining_self_loops(i["edge_index"].to(dev()), ew, num_nodes=x.size(0))
    with torch.no_grad(), Routes() as r:
        alpha, x_new, fit = p.fitness(x, ei, ew)
    assert r.native == 1
    torch.testing.assert_close(alpha.cpu(), e["alpha"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(x_new.cpu(), e["x_new"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(fit.cpu(), e["score"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(alpha.double().cpu(), c["f64"]["alpha"], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ graphs for the kernels
_graphs = {}


def graph(kind):
    """Host edge lists WITH their self-loops.  ``one``: a single node with only its loop.  ``small``: 257 nodes, 1536
    random edges (average in-degree 6), node 5 with no in-edge but its loop, 100 edges listed twice, shuffled.
    ``hub<d>``: ``small`` plus a hub (node 7) whose in-degree, loop included, is exactly d, shuffled; ``hub<d>g`` the
    same list stably sorted by destination (the offsets-only index).  64 is the lane count of the softmax kernel's edge
    loop and a multiple of every slot count of the row kernels, so 63 / 64 / 65 stand on both sides of their strides;
    3000 is a long walk of one wave."""
    if kind in _graphs:
        return _graphs[kind]
    if kind == "one":
        out = (torch.zeros(2, 1, dtype=torch.long), 1)
    else:
        g = torch.Generator().manual_seed(41)
        n = 257
        ei = torch.randint(0, n, (2, 1536), generator=g)
        ei = ei[:, (ei[1] != 5) & (ei[0] != ei[1])]
        ei = torch.cat([ei, ei[:, :100]], 1)
        if kind.startswith("hub"):
            d = int(kind[3:].rstrip("g"))
            ei = ei[:, ei[1] != 7]
            srcs = torch.randint(0, n, (4 * d + 8,), generator=g)
            srcs = srcs[srcs != 7][: d - 1]
            ei = torch.cat([ei, torch.stack([srcs, torch.full_like(srcs, 7)])], 1)
        ei, _ = R.add_remaining_self_loops(ei, None, n)
        ei = ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()
        if kind.endswith("g"):
            ei = ei[:, torch.argsort(ei[1], stable=True)].contiguous()
        indeg = torch.bincount(ei[1], minlength=n)
        assert int(indeg[5]) == 1 and (not kind.startswith("hub") or int(indeg[7]) == int(kind[3:].rstrip("g")))
        out = (ei, n)
    _graphs[kind] = out
    return out


GRAPHS = ["one", "small", "hub63", "hub64", "hub65", "hub65g", "hub3000", "hub3000g"]


def rows(n, f, strided, seed=0):
    g = torch.Generator().manual_seed(1000 * n + 10 * f + len(str(strided)) + seed)
    if strided == "unaligned":  # a column slice: row stride f + 3, base 4 bytes past a 16-byte boundary
        x = torch.randn(n, f + 3, generator=g).to(dev())[:, 1:1 + f]
        assert x.stride(0) == f + 3 and x.data_ptr() % 16 != 0
    elif strided == "aligned":  # a column slice that keeps the 16-byte loads
        x = torch.randn(n, (f + 7) // 4 * 4, generator=g).to(dev())[:, :f]
        assert x.stride(0) % 4 == 0 and x.stride(0) > f and x.data_ptr() % 16 == 0
    else:
        x = torch.randn(n, f, generator=g).to(dev())
    return x, g


def group_of(ei, n):
    ei_d = ei.to(dev())
    grp = K.sag_edge_group(ei_d, n, by_destination=True)
    return ei_d, grp


SHAPES = [(f, s) for f in (1, 3, 4, 5, 64, 67, 130) for s in (False, "unaligned", "aligned")]
SHAPE_IDS = [f"F{f}-{s or 'contiguous'}" for f, s in SHAPES]
CASES_K = [("hub65", f, s) for f, s in SHAPES] + [(k, f, False) for k in GRAPHS for f in (5, 64)]
IDS_K = [f"{k}-F{f}-{s or 'contiguous'}" for k, f, s in CASES_K]


# ------------------------------------------------------------------------------------------------ master query
@pytest.mark.parametrize("kind,f,strided", CASES_K, ids=IDS_K)
def test_query_against_float64(kind, f, strided):
    """|sq - (<max row, w~> + c)_64| <= (F + 4) 2^-24 (sum_f |m_f w~_f| + |c|).  The maximum is exact; the F products
    are fused into F additions (one rounding each), the lane fold and the column blocks (at most 3 here) are further
    additions of the same partial sums, adding c is one more: every rounding acts on a partial sum no larger than the
    sum of magnitudes, and no value passes through more than F + 4 of them."""
    ei, n = graph(kind)
    x, g = rows(n, f, strided)
    wt, c = torch.randn(f, generator=g).to(dev()), torch.randn(1, generator=g).to(dev())
    ei_d, grp = group_of(ei, n)
    assert (grp.perm is None) == kind.endswith("g") or kind == "one"
    sq = K.asap_query(grp, ei_d[0], x, wt, c)
    x64 = x.double().cpu()
    mx = R.scatter_max(x64[ei[0]], ei[1], n)
    want = mx @ wt.double().cpu() + c.double().cpu()
    bound = (f + 4) * U * (mx.abs() @ wt.double().cpu().abs() + c.double().cpu().abs())
    err = (sq.double().cpu() - want).abs()
    print(f"query {kind} F={f} {strided}: max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_query_takes_the_maximum_exactly_and_a_nan_wins():
    """w~ = e_f picks column f of the max row: the result is a row entry, bit for bit; a NaN among a node's candidates
    gives NaN (torch's amax), fmaxf alone would drop it; a node without in-edges gives c."""
    ei, n = graph("hub65")
    x, _ = rows(n, 6, False)
    ei_d, grp = group_of(ei, n)
    c = torch.zeros(1, device=dev())
    mx = R.scatter_max(x.cpu()[ei[0]], ei[1], n)
    for f in range(6):
        e = torch.zeros(6, device=dev())
        e[f] = 1.0
        assert torch.equal(K.asap_query(grp, ei_d[0], x, e, c).cpu(), mx[:, f] + 0.0)
    x[11, 2] = float("nan")
    got = K.asap_query(grp, ei_d[0], x, torch.ones(6, device=dev()), c).cpu()
    hit = torch.zeros(n, dtype=torch.bool)
    hit[ei[1][ei[0] == 11]] = True
    assert bool(got[hit].isnan().all()) and not bool(got[~hit].isnan().any())
    lone = torch.tensor([[0, 1], [1, 1]], device=dev())  # node 0 and node 2 have no in-edge
    got = K.asap_query(K.sag_edge_group(lone, 3), lone[0], x[:3], torch.ones(6, device=dev()), c + 0.25).cpu()
    assert got[0] == 0.25 and got[2] == 0.25


# ------------------------------------------------------------------------------------------------ edge softmax
@pytest.mark.parametrize("slope", [0.2, 0.0])
@pytest.mark.parametrize("kind", GRAPHS)
def test_edge_softmax_against_float64(kind, slope):
    """Against float64 on the kernel's own float32 sq and sp.  With L the largest |l| of the group and d its size:
    l = leaky(sq + sp) carries 2 roundings, l - m one more, so the exponent is off by at most 6 L 2^-24 and exp by that
    relative amount plus 2 ulp of expf; the sum of d such terms adds at most d roundings, the 1e-16 (below 2^-24 of a
    sum that is at least 1) and the division one each: |alpha - alpha_64| <= alpha_64 (d + 16 + 12 L) 2^-24."""
    ei, n = graph(kind)
    g = torch.Generator().manual_seed(3)
    sq, sp = torch.randn(n, generator=g).to(dev()) * 2, torch.randn(n, generator=g).to(dev()) * 2
    ei_d, grp = group_of(ei, n)
    alpha = K.asap_edge_softmax(grp, ei_d[0], sq, sp, slope)
    assert alpha.shape == (ei.size(1),)
    l = torch.nn.functional.leaky_relu(sq.double().cpu()[ei[1]] + sp.double().cpu()[ei[0]], slope)
    want = R.softmax(l, ei[1], n)
    d = torch.bincount(ei[1], minlength=n)[ei[1]]
    big = torch.zeros(n, dtype=torch.float64).scatter_reduce(0, ei[1], l.abs(), reduce="amax")[ei[1]]
    bound = want * (d + 16 + 12 * big) * U
    err = (alpha.double().cpu() - want).abs()
    print(f"softmax {kind} slope={slope}: max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    sums = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], alpha.double().cpu())
    assert float((sums - 1).abs().max()) < 1e-5
    assert float(alpha.cpu()[ei[1] == 5]) == 1.0 if n > 5 else float(alpha) == 1.0  # only the loop: exp(0) / (1 + 1e-16)


# ------------------------------------------------------------------------------------------------ attend
@pytest.mark.parametrize("kind,f,strided", CASES_K, ids=IDS_K)
def test_attend_against_float64(kind, f, strided):
    """|x_new - (sum_e alpha_e x[src_e])_64| <= (d + 2) 2^-24 sum_e |alpha_e x[src_e]| per entry: d fused
    multiply-adds, one rounding each, the slot fold being some of those additions in another order.  The projections
    are taken from the kernel's own float32 row: |p_k - <x_new, w_k>_64| <= (F + 4) 2^-24 sum_f |x_new_f w_kf|, as for
    the query.  Without ``val`` every edge counts 1; without ``proj`` no projection is written."""
    ei, n = graph(kind)
    x, g = rows(n, f, strided, seed=1)
    alpha = torch.rand(ei.size(1), generator=g).to(dev())
    w3 = torch.randn(3, f, generator=g).to(dev())
    ei_d, grp = group_of(ei, n)
    out, p = K.asap_attend(grp, ei_d[0], x, alpha, w3)
    assert out.shape == (n, f) and out.is_contiguous() and p.shape == (3, n)
    x64, a64 = x.double().cpu(), alpha.double().cpu().view(-1, 1)
    d = torch.bincount(ei[1], minlength=n).view(-1, 1)
    want = torch.zeros(n, f, dtype=torch.float64).index_add_(0, ei[1], a64 * x64[ei[0]])
    mag = torch.zeros(n, f, dtype=torch.float64).index_add_(0, ei[1], (a64 * x64[ei[0]]).abs())
    err = (out.double().cpu() - want).abs()
    print(f"attend {kind} F={f} {strided}: max err/bound {float((err / ((d + 2) * U * mag).clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= (d + 2) * U * mag).all())
    o64, w64 = out.double().cpu(), w3.double().cpu()
    perr = (p.double().cpu() - w64 @ o64.t()).abs()
    assert bool((perr <= (f + 4) * U * (w64.abs() @ o64.abs().t())).all())
    ones, none = K.asap_attend(grp, ei_d[0], x)
    assert none is None
    want1 = torch.zeros(n, f, dtype=torch.float64).index_add_(0, ei[1], x64[ei[0]])
    mag1 = torch.zeros(n, f, dtype=torch.float64).index_add_(0, ei[1], x64[ei[0]].abs())
    assert bool(((ones.double().cpu() - want1).abs() <= (d + 2) * U * mag1).all())


def test_attend_over_the_by_source_group_pulls_a_gradient_back():
    """The same kernel over the by-source index with dst as the gathered endpoint: g_x[j] = sum_{e out of j} alpha_e
    g[dst_e] -- what the backward of x_new needs; a table with another row count than the group's is allowed."""
    ei, n = graph("hub65")
    g = torch.Generator().manual_seed(8)
    gx_new = torch.randn(n, 12, generator=g).to(dev())
    alpha = torch.rand(ei.size(1), generator=g).to(dev())
    ei_d = ei.to(dev())
    by_src = K.sag_edge_group(ei_d, n, by_destination=False)
    got, _ = K.asap_attend(by_src, ei_d[1], gx_new, alpha)
    a64 = alpha.double().cpu().view(-1, 1)
    want = torch.zeros(n, 12, dtype=torch.float64).index_add_(0, ei[0], a64 * gx_new.double().cpu()[ei[1]])
    mag = torch.zeros(n, 12, dtype=torch.float64).index_add_(0, ei[0], (a64 * gx_new.double().cpu()[ei[1]]).abs())
    d = torch.bincount(ei[0], minlength=n).view(-1, 1)
    assert bool(((got.double().cpu() - want).abs() <= (d + 2) * U * mag).all())


def test_endpoints_out_of_range_are_skipped():
    d = dev()
    ei = torch.tensor([[0, 99, 2, -1, 3], [1, 1, 1, 3, 3]], device=d)
    x = torch.randn(4, 5, device=d)
    grp = K.sag_edge_group(ei, 4)
    out, _ = K.asap_attend(grp, ei[0], x)
    want = torch.zeros(4, 5, device=d)
    want[1], want[3] = x[0] + x[2], x[3]
    assert torch.equal(out, want)
    sq = K.asap_query(grp, ei[0], x, torch.tensor([1.0, 0, 0, 0, 0], device=d), torch.zeros(1, device=d))
    assert float(sq[1]) == float(torch.maximum(x[0, 0], x[2, 0])) and float(sq[3]) == float(x[3, 0])
    alpha = K.asap_edge_softmax(grp, ei[0], torch.zeros(4, device=d), torch.zeros(4, device=d), 0.2)
    assert alpha.tolist() == [0.5, 0.0, 0.5, 0.0, 1.0]
    p = torch.randn(3, 4, device=d)
    t = K.asap_leconv(grp, ei[0], p)
    assert float(t[1]) == float((p[2, 1] + (p[0, 0] + p[0, 2])) + (0.0 - p[1, 1]) * 2.0)


# ------------------------------------------------------------------------------------------------ LEConv aggregate
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kind", GRAPHS)
def test_leconv_against_float64(kind, weighted):
    """t = ((p3 + b3) + s) + (b1 - p2) W with s = sum_e w_e p1[src_e] (d fused multiply-adds) and W = sum_e w_e (d
    additions): |t - t_64| <= (d + 6) 2^-24 (|p3| + |b3| + sum_e |w_e p1| + (|b1| + |p2|) sum_e |w_e|) -- d roundings in
    either sum, then the subtraction, the product and three additions.  tanh: 4 ulp of a value below 1; sigmoid
    1 / (1 + exp(-t)): expf, one addition, one division, below 8 * 2^-24."""
    ei, n = graph(kind)
    g = torch.Generator().manual_seed(13)
    p = torch.randn(3, n, generator=g).to(dev())
    ew = (torch.rand(ei.size(1), generator=g) + 0.1).to(dev()) if weighted else None
    b1, b3 = torch.tensor([0.3]).to(dev()), torch.tensor([-0.7]).to(dev())
    ei_d, grp = group_of(ei, n)
    t, a = K.asap_leconv(grp, ei_d[0], p, ew, b1, b3, "sigmoid", want_t=True)
    p64 = p.double().cpu()
    w64 = torch.ones(ei.size(1), dtype=torch.float64) if ew is None else ew.double().cpu()
    s = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], w64 * p64[0][ei[0]])
    smag = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], (w64 * p64[0][ei[0]]).abs())
    wsum = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], w64)
    b1d, b3d = float(b1.double().cpu()), float(b3.double().cpu())
    want = p64[2] + b3d + s + (b1d - p64[1]) * wsum
    d = torch.bincount(ei[1], minlength=n)
    bound = (d + 6) * U * (p64[2].abs() + abs(b3d) + smag + (abs(b1d) + p64[1].abs()) * wsum)
    err = (t.double().cpu() - want).abs()
    print(f"leconv {kind} weighted={weighted}: max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert float((a.double().cpu() - torch.sigmoid(t.double().cpu())).abs().max()) <= 8 * U
    th = K.asap_leconv(grp, ei_d[0], p, ew, b1, b3, "tanh")
    assert float((th.double().cpu() - torch.tanh(t.double().cpu())).abs().max()) <= 4 * U
    assert torch.equal(K.asap_leconv(grp, ei_d[0], p, ew, b1, b3), t)


def test_leconv_module_scores_natively_and_matches_its_composed_form():
    ei, n = graph("hub65")
    torch.manual_seed(5)
    conv = LEConv(9, 1)
    x = torch.randn(n, 9)
    ew = torch.rand(ei.size(1)) + 0.1
    with torch.no_grad():
        want = conv(x, ei, ew).view(-1)
        conv_d = conv.to(dev())
        got = conv_d.score(x.to(dev()), ei.to(dev()), ew.to(dev()))
        col = conv_d(x.to(dev()), ei.to(dev()), ew.to(dev()))
    assert got is not None and col.shape == (n, 1)
    torch.testing.assert_close(got.cpu(), want, rtol=1e-5, atol=1e-5)
    assert torch.equal(col.view(-1), got)
    tracked = conv_d.score(x.to(dev()).requires_grad_(True), ei.to(dev()))
    assert type(tracked.grad_fn).__name__ == "_AsapLeconvFnBackward"
    assert conv_d.score(x.to(dev()), ei.to(dev()), ew.to(dev()).requires_grad_(True)) is None  # no gradient for weights


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("kind", ["hub3000", "hub3000g"])
def test_the_fitness_is_bit_identical_run_to_run(kind):
    ei, n = graph(kind)
    torch.manual_seed(2)
    pool = ASAPooling(32).to(dev()).eval()
    x = torch.randn(n, 32, generator=torch.Generator().manual_seed(6)).to(dev())
    ew = (torch.rand(ei.size(1), generator=torch.Generator().manual_seed(7)) + 0.1).to(dev())
    with torch.no_grad():
        first = pool.fitness(x, ei.to(dev()), ew, act="sigmoid")
        K._SAG_GROUPS.clear()  # the second call rebuilds its index as well
        second = pool.fitness(x, ei.to(dev()), ew, act="sigmoid")
    for a, b in zip(first, second):
        assert torch.equal(a, b)

    def grads():
        K._SAG_GROUPS.clear()
        xg = x.clone().requires_grad_(True)
        _, x_new, score = pool.fitness(xg, ei.to(dev()), ew, act="sigmoid")
        leaves = [xg] + list(pool.parameters())
        return torch.autograd.grad((x_new * score.view(-1, 1)).square().sum(), leaves)

    for a, b in zip(grads(), grads()):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ dropout mask
def test_a_mask_on_alpha_matches_the_restatement_under_the_same_mask():
    c = CASES["asap_weighted"]
    p = build(c)
    i = c["inputs"]
    x = i["x"].to(dev())
    ei, ew = add_remaining_self_loops(i["edge_index"].to(dev()), i["edge_weight"].to(dev()), num_nodes=x.size(0))
    mask = torch.nn.functional.dropout(torch.ones(ei.size(1)), p=0.4, training=True)
    assert 0 < int((mask == 0).sum()) < mask.numel()
    with torch.no_grad(), Routes() as r:
        alpha, x_new, fit = p.fitness(x, ei, ew, mask=mask.to(dev()))
    assert r.native == 1
    want = R.pool_case(c, torch.float64, mask=mask.double())
    torch.testing.assert_close(alpha.double().cpu(), want["alpha"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(x_new.double().cpu(), want["x_new"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(fit.double().cpu(), want["fitness"], rtol=1e-5, atol=1e-5)
    # training mode draws its own mask on the native route: the dropped edges are exact zeros, the kept ones scaled
    p.train()
    p.dropout = 0.4
    torch.manual_seed(0)
    with torch.no_grad(), Routes() as r:
        alpha_t, _, _ = p.fitness(x, ei, ew)
    assert r.native == 1 and 0 < int((alpha_t == 0).sum()) < alpha_t.numel()


# ------------------------------------------------------------------------------------------------ memory
def test_the_native_fitness_forms_no_e_by_f_temporary():
    """N = 4096, E = 262144, F = 256: an E x F matrix is 268 MB.  One cold call builds the augmented list and the
    by-destination index (both remembered); the warm no-grad attention + score may then rise by less than E F 4 / 4
    bytes = 64 MB above what was allocated before it (x_new is 4 MB, the E'-sized vectors about 1 MB each)."""
    n, E, F = 4096, 262144, 256
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, F, generator=g).to(dev())
    ei = torch.randint(0, n, (2, E), generator=g).to(dev())
    torch.manual_seed(1)
    pool = ASAPooling(F).to(dev()).eval()
    with torch.no_grad():
        ea, _ = add_remaining_self_loops(ei, None, num_nodes=n)
        warm = pool.fitness(x, ea, None, act="sigmoid")
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ea2, _ = add_remaining_self_loops(ei, None, num_nodes=n)
        with Routes() as r:
            again = pool.fitness(x, ea2, None, act="sigmoid")
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    print(f"fitness call: peak rise {rise} bytes (E*F*4 = {E * F * 4})")
    assert ea2 is ea and r.native == 1
    assert all(torch.equal(a, b) for a, b in zip(warm, again))
    assert rise < E * F * 4 // 4


# ------------------------------------------------------------------------------------------------ non-finite inputs
def test_non_finite_rows_follow_the_composed_form():
    """One x row with a NaN and one with +inf: the NaN masks and the signed infinities of x_new and of
    the fitness equal those of the composed form on the host; the finite rest agrees at 1e-5."""
    c = CASES["asap_directed"]
    i = c["inputs"]
    x = i["x"].clone()
    x[3, 1] = float("nan")
    x[20, 2] = float("inf")
    host = build(c).cpu()
    ei_h, _ = add_remaining_self_loops(i["edge_index"], None, num_nodes=x.size(0))
    with torch.no_grad():
        want = host.fitness(x, ei_h, None)
        p = build(c)
        with Routes() as r:
            got = p.fitness(x.to(dev()), ei_h.to(dev()), None)
    assert r.native == 1
    for name, g, w in zip(("alpha", "x_new", "fitness"), got, want):
        g = g.cpu()
        assert torch.equal(g.isnan(), w.isnan()), name
        assert torch.equal(g.isinf(), w.isinf()) and torch.equal(g[g.isinf()], w[w.isinf()]), name
        fin = g.isfinite()
        assert 0 < int(fin.sum()) < g.numel(), name
        torch.testing.assert_close(g[fin], w[fin], rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ routing
@pytest.mark.parametrize("name", ["asap_weighted", "asap_self_loops_unsorted"])
def test_float64_inputs_and_weight_gradients_take_the_composed_form(name):
    c = CASES[name]
    with Routes() as r, torch.no_grad():
        out = forward(build(c, dtype=torch.float64), c, dtype=torch.float64)
    assert r.native == 0 and out.x.dtype == torch.float64
    check_output(out, c["expected"], name)
    torch.testing.assert_close(out.x.cpu(), c["f64"]["x"], rtol=1e-9, atol=1e-9)
    with Routes() as r:
        out = forward(build(c), c, ew_grad=True)
    assert r.native == 0
    check_output(out, c["expected"], name)


def test_nothing_is_remembered_while_a_stream_is_capturing():
    c = CASES["asap_weighted"]
    p = build(c)
    i = c["inputs"]
    x = i["x"].to(dev())
    ei, ew = i["edge_index"].to(dev()), i["edge_weight"].to(dev())
    with torch.no_grad():
        ea, wa = add_remaining_self_loops(ei, ew, num_nodes=x.size(0))
        eager = p.fitness(x, ea, wa, act="sigmoid")  # warms the edge group of the augmented list
        torch.cuda.synchronize()
        O._LOOPED_EDGES.clear()
        before = (len(O._LOOPED_EDGES), len(K._SAG_GROUPS))
        graph_ = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            p.fitness(x, ea, wa, act="sigmoid")  # the capture's allocations come from a warmed pool
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph_):
            captured = p.fitness(x, ea, wa, act="sigmoid")
        assert (len(O._LOOPED_EDGES), len(K._SAG_GROUPS)) == before
        graph_.replay()
        torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
    again = add_remaining_self_loops(ei, ew, num_nodes=x.size(0))  # outside a capture the list is remembered again
    assert add_remaining_self_loops(ei, ew, num_nodes=x.size(0))[0] is again[0]


# ------------------------------------------------------------------------------------------------ backward kernels
@pytest.mark.parametrize("kind", ["small", "hub65", "hub65g", "hub3000"])
def test_argmax_positions_are_exact_and_ties_go_to_the_lower_position(kind):
    """Duplicate edges (100 of them in every list) tie in every column, and rows 20 and 21 are made equal to plant ties
    between different sources: the stored positions equal the restatement's, which takes the lowest."""
    ei, n = graph(kind)
    x, _ = rows(n, 7, False)
    x[21] = x[20]
    x[30, 3] = x[31, 3]
    ei_d, grp = group_of(ei, n)
    wt, c = torch.ones(7, device=dev()), torch.zeros(1, device=dev())
    sq, arg = K.asap_query(grp, ei_d[0], x, wt, c, want_arg=True)
    mx, want = R.master_query(x.cpu(), ei, n)
    assert arg.dtype == torch.int32 and torch.equal(arg.cpu().long(), want)
    assert torch.equal(sq, K.asap_query(grp, ei_d[0], x, wt, c))
    picked = x.cpu()[ei[0][want], torch.arange(7).expand(n, 7)]
    assert torch.equal(picked, mx)
    dup = torch.unique(ei, dim=1).size(1)
    assert dup < ei.size(1)


@pytest.mark.parametrize("kind,f,strided", CASES_K, ids=IDS_K)
def test_edge_dot_against_float64(kind, f, strided):
    """|out_e - <g[dst_e], x[src_e]>_64| <= (F + 2) 2^-24 sum_f |g_f x_f|: F fused multiply-adds and the lane fold."""
    ei, n = graph(kind)
    x, gen = rows(n, f, strided, seed=2)
    g = torch.randn(n, f, generator=gen).to(dev())
    ei_d, grp = group_of(ei, n)
    out = K.asap_edge_dot(grp, ei_d[0], g, x)
    g64, x64 = g.double().cpu(), x.double().cpu()
    want = (g64[ei[1]] * x64[ei[0]]).sum(1)
    bound = (f + 2) * U * (g64[ei[1]] * x64[ei[0]]).abs().sum(1)
    assert bool(((out.double().cpu() - want).abs() <= bound).all())


@pytest.mark.parametrize("slope", [0.2, 0.0])
@pytest.mark.parametrize("kind", GRAPHS)
def test_softmax_bwd_against_float64(kind, slope):
    """Against float64 on the kernel's own float32 alpha: d = sum alpha g_alpha costs at most (deg + 1) roundings of
    sum |alpha g_alpha| =: D; g_l = alpha (g_alpha - d) s then three more on a value below alpha (|g_alpha| + D):
    |g_l - g_l_64| <= alpha ((deg + 2) D + 3 (|g_alpha| + D)) 2^-24, and g_sq sums deg of them:
    |g_sq - g_sq_64| <= sum_e bound_e + (deg + 1) 2^-24 sum_e |g_l|."""
    ei, n = graph(kind)
    gen = torch.Generator().manual_seed(17)
    sq, sp = torch.randn(n, generator=gen).to(dev()), torch.randn(n, generator=gen).to(dev())
    g_alpha = torch.randn(ei.size(1), generator=gen).to(dev())
    ei_d, grp = group_of(ei, n)
    alpha = K.asap_edge_softmax(grp, ei_d[0], sq, sp, slope)
    g_l, g_sq = K.asap_softmax_bwd(grp, ei_d[0], alpha, g_alpha, sq, sp, slope)
    a64, ga64 = alpha.double().cpu(), g_alpha.double().cpu()
    t = sq.cpu()[ei[1]] + sp.cpu()[ei[0]]  # the float32 sum whose sign the kernel tests
    d = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], a64 * ga64)
    D = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], (a64 * ga64).abs())
    scale = torch.where(t > 0, 1.0, slope).double()
    want = a64 * (ga64 - d[ei[1]]) * scale
    deg = torch.bincount(ei[1], minlength=n)
    bound = a64 * ((deg[ei[1]] + 2) * D[ei[1]] + 3 * (ga64.abs() + D[ei[1]])) * U
    assert bool(((g_l.double().cpu() - want).abs() <= bound).all())
    want_sq = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], want)
    bound_sq = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], bound) + (deg + 1) * U * torch.zeros(
        n, dtype=torch.float64).index_add_(0, ei[1], want.abs())
    assert bool(((g_sq.double().cpu() - want_sq).abs() <= bound_sq).all())


@pytest.mark.parametrize("f", [1, 5, 64, 67])
@pytest.mark.parametrize("kind", ["small", "hub65", "hub65g", "hub3000"])
def test_query_bwd_against_float64(kind, f):
    """out[j,f] = w~_f sum of g_sq[dst] over j's out-edges that hold the arg-max of (dst, f): at most outdeg additions and
    one product, |out - out_64| <= (outdeg + 2) 2^-24 |w~_f| sum |g_sq[dst]| over those edges."""
    ei, n = graph(kind)
    x, gen = rows(n, f, False, seed=3)
    wt, g_sq = torch.randn(f, generator=gen).to(dev()), torch.randn(n, generator=gen).to(dev())
    ei_d, grp = group_of(ei, n)
    _, arg = K.asap_query(grp, ei_d[0], x, wt, torch.zeros(1, device=dev()), want_arg=True)
    by_src = K.sag_edge_group(ei_d, n, by_destination=False)
    out = K.asap_query_bwd(by_src, ei_d[1], arg, g_sq, wt)
    a = arg.cpu().long()
    want = torch.zeros(n, f, dtype=torch.float64)
    mag = torch.zeros(n, f, dtype=torch.float64)
    cols = torch.arange(f).expand(n, f)
    gq = g_sq.double().cpu().view(-1, 1).expand(n, f)
    want.index_put_((ei[0][a].reshape(-1), cols.reshape(-1)), gq.reshape(-1), accumulate=True)
    mag.index_put_((ei[0][a].reshape(-1), cols.reshape(-1)), gq.abs().reshape(-1), accumulate=True)
    w64 = wt.double().cpu()
    outdeg = torch.bincount(ei[0], minlength=n).view(-1, 1)
    assert bool(((out.double().cpu() - want * w64).abs() <= (outdeg + 2) * U * mag * w64.abs()).all())


# ------------------------------------------------------------------------------------------------ gradients
def _fitness_paths(pool_state, cfg, x0, ei, ew, mask=None):
    """kernel / oracle closures for check_grad_paths: x_new alone, the activated score alone, and sum((x_new s)^2)."""
    names = sorted(pool_state)

    def kernel():
        p = ASAPooling(**cfg).to(dev())
        p.load_state_dict(pool_state)
        x = x0.to(dev()).requires_grad_(True)
        with Routes() as r:
            _, x_new, score = p.fitness(x, ei.to(dev()), None if ew is None else ew.to(dev()),
                                        mask=None if mask is None else mask.to(dev()), act="sigmoid")
        assert r.native == 1 and type(score.grad_fn).__name__ == "_AsapLeconvFnBackward"
        lv = {"x": x, **{k: dict(p.named_parameters())[k] for k in names}}
        return {"x_new": x_new, "score": score, "sum_sq": ((x_new * score.view(-1, 1)) ** 2).sum()}, lv

    def oracle(dtype):
        x = x0.to(dtype).requires_grad_(True)
        par = {k: v.to(dtype).requires_grad_(True) for k, v in pool_state.items()}
        _, x_new, fit = R.fitness_reference_shaped(x, x, ei, None if ew is None else ew.to(dtype), par,
                                                   cfg.get("negative_slope", 0.2),
                                                   None if mask is None else mask.to(dtype))
        score = torch.sigmoid(fit)
        return {"x_new": x_new, "score": score, "sum_sq": ((x_new * score.view(-1, 1)) ** 2).sum()}, {"x": x, **par}

    return kernel, oracle, ["x"] + names


@pytest.mark.parametrize("kind", ["hub3000", "hub65g"])
def test_gradients_of_the_fitness_on_the_hub_graph(kind):
    """x, lin, att and LEConv's five parameters, one upstream path at a time, against the float64 reference-shaped
    restatement with its float32 run as the measure of fp32's own error."""
    ei, n = graph(kind)
    torch.manual_seed(12)
    state = {k: v.clone() for k, v in ASAPooling(8).state_dict().items()}
    x0 = torch.randn(n, 8, generator=torch.Generator().manual_seed(14))
    ew = torch.rand(ei.size(1), generator=torch.Generator().manual_seed(15)) + 0.1
    kernel, oracle, leaves = _fitness_paths(state, dict(in_channels=8), x0, ei, ew)
    check_grad_paths(f"asap/{kind}", kernel, oracle, leaves)


def test_gradients_of_the_fitness_on_a_directed_batch_with_duplicates_and_a_mask():
    c = CASES["asap_duplicates"]
    i = c["inputs"]
    ei, _ = R.add_remaining_self_loops(i["edge_index"], None, i["x"].size(0))
    mask = torch.nn.functional.dropout(torch.ones(ei.size(1)), p=0.3, training=True)
    for m in (None, mask):
        kernel, oracle, leaves = _fitness_paths(c["params"], c["cfg"], i["x"], ei, None, m)
        check_grad_paths(f"asap/duplicates/mask={m is not None}", kernel, oracle, leaves)


@pytest.mark.parametrize("name", ["asap_weighted", "asap_gnn", "asap_tanh", "asap_one_column"])
def test_gradients_of_the_pooler_match_the_fixture(name):
    """The fixture's objective sum(x_pool^2) through the whole public class: x and every parameter against the stored
    float64 gradients, with the float64 restatement's float32 run as the measure (test_asap_restatement.py pins the
    restatement to the same stored gradients at 1e-12)."""
    c = CASES[name]
    names = sorted(c["params"])

    def kernel():
        p = build(c, requires_grad=True)
        i = c["inputs"]
        x = i["x"].to(dev()).requires_grad_(True)
        ew = None if i["edge_weight"] is None else i["edge_weight"].to(dev())
        with Routes() as r:
            out = p(x=x, adj=i["edge_index"].to(dev()), edge_weight=ew,
                    batch=None if i["batch"] is None else i["batch"].to(dev()))
        assert r.native == 1
        return {"sum_sq": (out.x ** 2).sum()}, {"x": x, **{k: dict(p.named_parameters())[k] for k in names}}

    def oracle(dtype):
        x = c["inputs"]["x"].to(dtype).requires_grad_(True)
        par = {k: v.to(dtype).requires_grad_(True) for k, v in c["params"].items()}
        got = R.pool_case(c, dtype, collapsed=False, params=par, x=x)
        return {"sum_sq": (got["x_pool"] ** 2).sum()}, {"x": x, **par}

    check_grad_paths(name, kernel, oracle, ["x"] + names)


# ------------------------------------------------------------------------------------------------ regressions of the sweep
def test_a_list_without_edges_goes_through_the_backward():
    """The sweep's (asap, seed 11, g_sq) and (asap, seed 12, g_sq): five graphs without a single edge (224 nodes,
    F = 16).  With E = 0 every per-edge pointer of ``asap_softmax_bwd`` is NULL, and the entry took the two NULLs of
    ``g_l`` and ``alpha`` for "an input given as an output": the backward of the attention raised; past it, the node
    looked the maxima's source rows up in an empty ``row``.  The operator gives an empty g_l and g_sq = 0; the two nodes'
    gradients are those of the float64 reference-shaped restatement (x_new = 0, every node's query is the bias row)."""
    n, f = 224, 16
    gen = torch.Generator().manual_seed(11)
    ei = torch.zeros(2, 0, dtype=torch.long, device=dev())
    grp = K.sag_edge_group(ei, n, by_destination=True)
    none = torch.zeros(0, device=dev())
    g_l, g_sq = K.asap_softmax_bwd(grp, ei[0], none, none, torch.randn(n, generator=gen).to(dev()),
                                   torch.randn(n, generator=gen).to(dev()), 0.2)
    assert g_l.shape == (0,) and torch.equal(g_sq, torch.zeros(n, device=dev()))
    torch.manual_seed(11)
    state = {k: v.clone() for k, v in ASAPooling(f).state_dict().items()}
    x0 = torch.randn(n, f, generator=gen)
    kernel, oracle, leaves = _fitness_paths(state, dict(in_channels=f), x0, ei.cpu(), None)
    check_grad_paths("asap/no-edges", kernel, oracle, leaves)
