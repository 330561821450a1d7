"""MaxCutPooling on the MI355X: the public class against the reference's stored results, each kernel alone against
float64 with a bound derived from its arithmetic (never tuned), the assignment rounds exactly against the composed
routine, run-to-run determinism of results and gradients, gradients one upstream path at a time at fp32's own error (the
helper of test_gpu_grad_paths.py), the memory the native route may not take (nothing of size E x C), non-finite inputs
against the composed form, and which inputs take which route.  Without the feature this module fails at import."""
import os
import warnings

import pytest
import torch

import maxcut_restatement as R
from test_gpu_grad_paths import check_grad_paths

from tgp import functions as Fn
from tgp import kernels as K
from tgp.poolers import MaxCutPooling, MaxCutScoreNet, MaxCutSelect
from tgp.select import SelectOutput
from tgp.utils import maxcut_loss
from tgp.utils import ops as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_maxcut_v1.pt"), weights_only=True)["cases"]
POOL = sorted(n for n, c in CASES.items() if c["kind"] == "pool")
U = 2.0 ** -24  # fp32 unit roundoff
ACT_ULPS = 4  # tanhf on the device is within 2 ulp; relu and the identity are exact


def dev():
    return torch.device("cuda:0")


def build(c, requires_grad=False, dtype=torch.float32):
    p = MaxCutPooling(**c["cfg"]).eval()
    p.load_state_dict(c["params"])
    p = p.to(dev(), dtype)
    for q in p.parameters():
        q.requires_grad_(requires_grad)
    return p


def forward(p, c, dtype=torch.float32, ew_grad=False, x=None):
    i = c["inputs"]
    d = dev()
    ew = None if i["edge_weight"] is None else i["edge_weight"].to(d, dtype).requires_grad_(ew_grad)
    return p(x=i["x"].to(d, dtype) if x is None else x, adj=i["edge_index"].to(d), edge_weight=ew,
             batch=None if i["batch"] is None else i["batch"].to(d))


class Routes:
    """Counts the calls of the native score net, loss and assignment rounds while a block runs."""

    def __enter__(self):
        self.score = self.loss = self.rounds = 0
        self._orig = (Fn.maxcut_score, Fn.maxcut_loss, K.maxcut_assign_rounds)

        def score(*a, **k):
            self.score += 1
            return self._orig[0](*a, **k)

        def loss(*a, **k):
            self.loss += 1
            return self._orig[1](*a, **k)

        def rounds(*a, **k):
            self.rounds += 1
            return self._orig[2](*a, **k)

        Fn.maxcut_score, Fn.maxcut_loss, K.maxcut_assign_rounds = score, loss, rounds
        return self

    def __exit__(self, *exc):
        Fn.maxcut_score, Fn.maxcut_loss, K.maxcut_assign_rounds = self._orig


# ------------------------------------------------------------------------------------------------ the public class
@pytest.mark.parametrize("grad", [False, True], ids=["no_grad", "grad"])
@pytest.mark.parametrize("name", POOL)
def test_fixture_parity_through_the_public_class(name, grad):
    c = CASES[name]
    e, tol = c["expected"], 1e-5
    p = build(c, requires_grad=grad)
    with Routes() as r, torch.set_grad_enabled(grad):
        out = forward(p, c)
    assert (r.score, r.loss, r.rounds) == (1, 1, 1), "the three native parts run"
    so = out.so
    assert out.x.requires_grad == grad and so.scores.requires_grad == grad
    assert torch.equal(so.node_index.cpu(), e["so"]["node_index"]), name
    assert torch.equal(so.cluster_index.cpu(), e["so"]["cluster_index"]), name
    assert so.num_nodes == e["so"]["num_nodes"] and so.num_supernodes == e["so"]["num_supernodes"]
    assert torch.equal(out.edge_index.cpu(), e["edge_index"]), name
    assert out.batch is None if e["batch"] is None else torch.equal(out.batch.cpu(), e["batch"])
    torch.testing.assert_close(so.scores.detach().cpu(), e["scores"], rtol=tol, atol=tol)
    torch.testing.assert_close(so.weight.detach().cpu(), e["so"]["weight"], rtol=tol, atol=tol)
    torch.testing.assert_close(out.x.detach().cpu(), e["x"], rtol=tol, atol=tol)
    if e["edge_weight"] is None:
        assert out.edge_weight is None
    else:
        torch.testing.assert_close(out.edge_weight.detach().cpu(), e["edge_weight"], rtol=tol, atol=tol)
    assert sorted(out.loss) == ["maxcut_loss"]
    torch.testing.assert_close(out.loss["maxcut_loss"].detach().cpu(), e["loss"]["maxcut_loss"], rtol=tol, atol=tol)


@pytest.mark.parametrize("name,launches", [("maxcut_weighted", 1), ("maxcut_no_assign_all", 0)])
def test_a_batch_of_small_graphs_reduces_and_connects_in_one_launch(name, launches, monkeypatch):
    """The full weighted assignment is the shape the one-launch Reduce + Connect takes; with ``assign_all_nodes=False``
    Reduce and Connect read two different assignments and stay staged."""
    c = CASES[name]
    calls, real = [], K.sparse_pool_small

    def counted(*a, **k):
        out = real(*a, **k)
        calls.append(out is not None)
        return out

    monkeypatch.setattr(K, "sparse_pool_small", counted)
    with torch.no_grad():
        out = forward(build(c), c)
    assert calls == [True] * launches
    torch.testing.assert_close(out.x.cpu(), c["expected"]["x"], rtol=1e-5, atol=1e-5)


def test_the_empty_edge_list_scores_and_pools():
    c = CASES["maxcut_empty"]
    p = build(c)
    with torch.no_grad(), Routes() as r:
        out = forward(p, c)
    assert r.score == 1 and r.loss == 1
    torch.testing.assert_close(out.so.scores.cpu(), c["expected"]["scores"], rtol=1e-5, atol=1e-5)
    assert float(out.loss["maxcut_loss"]) == 0.0 and out.edge_index.size(1) == 0
    sizes = torch.bincount(c["inputs"]["batch"])
    assert out.x.size(0) == int(torch.ceil(sizes.float() * 0.5).sum())


# ------------------------------------------------------------------------------------------------ graphs for the kernels
_graphs = {}
HUB = {0: 3000, 1: 0, 2: 1, 3: 63, 4: 64, 5: 65}  # node -> its in-degree without self-loops


def graph(kind):
    """Host edge list of 3015 nodes.  Nodes 0 .. 5 have in-degrees 3000, 0, 1, 63, 64, 65 (64 is a multiple of every slot
    count of the layer kernel and the lane count of the one-lane-per-edge walks, so 63 / 64 / 65 stand on both sides of
    their strides; 3000 is a long walk of one wave), node 6 has two self-loops and nothing else, node 7 gets 8 -> 7 five
    times and 9 -> 7 twice, the other nodes up to 3012 have random in-edges (three each) and some self-loops, and nodes
    3013 and 3014 lie above every endpoint (n_P = 3013).  ``sorted``: stably sorted by destination (offsets only);
    ``shuffled``: the same multiset in random order (the permutation route); ``flipped``: the shuffled list
    with its two rows exchanged, so the OUT-degrees are 3000, 0, 1, 63, 64, 65 (the by-source walks of the degree and cut
    kernels cross the same strides)."""
    if kind in _graphs:
        return _graphs[kind]
    g = torch.Generator().manual_seed(41)
    n, top = 3015, 3013
    src, dst = [], []
    for node, d in HUB.items():
        s = torch.randint(10, top, (d,), generator=g)
        src.append(s)
        dst.append(torch.full((d,), node))
    src += [torch.tensor([6, 6]), torch.tensor([8, 9, 8, 8, 9, 8, 8])]
    dst += [torch.tensor([6, 6]), torch.full((7,), 7)]
    rest = torch.arange(8, top).repeat_interleave(3)
    rs = torch.randint(0, top, (rest.numel(),), generator=g)
    rs = torch.where((rs == 1) | (rs == 6), torch.full_like(rs, 11), rs)  # node 6 keeps its loops only, node 1 no edge
    src += [rs, torch.arange(20, 400, 7), torch.tensor([top - 1])]
    dst += [rest, torch.arange(20, 400, 7), torch.tensor([12])]
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    ei = ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()
    if kind == "sorted":
        ei = ei[:, torch.argsort(ei[1], stable=True)].contiguous()
    nl = ei[:, ei[0] != ei[1]]
    indeg = torch.bincount(nl[1], minlength=n)
    assert all(int(indeg[k]) == v for k, v in HUB.items()) and int(indeg[6]) == 0 and int(ei.max()) == top - 1
    assert not bool((ei == 1).any()) and bool(((ei[0] == ei[1]) & (ei[0] > 19)).any())
    if kind == "flipped":
        ei = ei.flip(0).contiguous()
    _graphs[kind] = (ei, n)
    return _graphs[kind]


def weights(ei, seed=5):
    return torch.rand(ei.size(1), generator=torch.Generator().manual_seed(seed)) + 0.1


def groups(ei, n):
    d = ei.to(dev())
    return d, K.sag_edge_group(d, n, by_destination=True), K.sag_edge_group(d, n, by_destination=False)


def out_terms(ei, n):
    """long [n]: the number of terms of every node's degree sum."""
    nl = ei[:, ei[0] != ei[1]]
    return torch.bincount(nl[0], minlength=n)


# ------------------------------------------------------------------------------------------------ degrees
@pytest.mark.parametrize("kind", ["shuffled", "flipped"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
def test_degree_kernel_against_float64(weighted, kind):
    """dinv: a sum of m terms spread over 64 lanes (lane l adds entries l, l + 64, ..) and six folds, a square root and a
    division -> (m + 6 + 3) u relative; a coefficient one product more.  ``flipped`` gives the by-source groups the
    lengths 0, 1, 63, 64, 65 and 3000: several partial sums per lane before the fold."""
    ei, n = graph(kind)
    w = weights(ei) if weighted else None
    d, _, by_src = groups(ei, n)
    dinv, coef, coef_t = K.maxcut_degree(by_src, d, None if w is None else w.to(dev()), True, True)
    w64 = torch.ones(ei.size(1), dtype=torch.float64) if w is None else w.double()
    ref = R.dinv_of(ei, w64, n)
    m = out_terms(ei, n).double()
    err = (dinv.cpu().double() - ref).abs()
    if kind == "flipped":
        assert [int(m[k]) for k in range(6)] == [3000, 0, 1, 63, 64, 65]
    assert bool((err <= (m + 9) * U * ref).all()), float((err / ref.clamp(min=1e-30)).max())
    assert bool((dinv.cpu()[m == 0] == 0).all()) and float(dinv[1]) == 0.0 and float(dinv[6]) == 0.0  # inf -> 0
    for got, end in ((coef, 0), (coef_t, 1)):
        want = w64 * ref[ei[end]]
        assert bool(((got.cpu().double() - want).abs() <= (m[ei[end]] + 10) * U * want).all())


def test_degree_kernel_has_the_same_bits_on_both_index_routes():
    """The shuffled list (permutation route) against its own stable sort by source (offsets only)."""
    eh, n = graph("shuffled")
    w = weights(eh)
    order = torch.argsort(eh[0], stable=True)
    eg = eh[:, order].contiguous()
    dh, _, src_h = groups(eh, n)
    dg, _, src_g = groups(eg, n)
    assert src_h.perm is not None and src_g.perm is None
    a = K.maxcut_degree(src_h, dh, w.to(dev()), True, True)
    b = K.maxcut_degree(src_g, dg, w[order].contiguous().to(dev()), True, True)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1][order.to(dev())], b[1]) and torch.equal(a[2][order.to(dev())], b[2])


# ------------------------------------------------------------------------------------------------ one layer
def layer_inputs(kind, C, seed=3):
    ei, n = graph(kind)
    g = torch.Generator().manual_seed(seed)
    return ei, n, torch.randn(n, C, generator=g), torch.randn(C, generator=g) * 0.5


@pytest.mark.parametrize("act", ["tanh", "relu", "identity"])
@pytest.mark.parametrize("C", [1, 5, 8, 16, 32, 33, 64])
def test_layer_kernel_against_float64(C, act):
    """Entry (i, c): T = delta dinv_i sum |w dinv_r z_r| + |(1 - delta) z_i| + |b|.  The sum has m_i terms (a slot adds
    them in order, at most log2(64) folds follow), every term carries the two dinv factors ((D + 3) u each, D the most
    terms of a degree sum) and three products, the diagonal term one product, two additions follow:
    |t - t_64| <= (m_i + 2 D + 6 + 12 + 4) u T; the activation is 1-Lipschitz and adds ACT_ULPS u |h|."""
    ei, n, z, b = layer_inputs("shuffled", C)
    w = weights(ei)
    d, by_dst, by_src = groups(ei, n)
    dinv, coef, _ = K.maxcut_degree(by_src, d, w.to(dev()))
    n_p = K.maxcut_n_p(d)
    assert int(n_p) == 3013
    h, zn = K.maxcut_layer(by_dst, d[0], coef, dinv, z.to(dev()), b.to(dev()), n_p, 2.0, act)
    assert zn is None and h.shape == (n, C)
    w64, z64 = w.double(), z.double()
    dinv64 = R.dinv_of(ei, w64, n)
    ref = R.layer_collapsed(z64, ei, w64, dinv64, 3013, 2.0, b.double(), act)
    keep = ei[0] != ei[1]
    mag = torch.zeros(n, C, dtype=torch.float64).index_add(
        0, ei[1][keep], (z64[ei[0][keep]] * (w64[keep] * dinv64[ei[0][keep]]).view(-1, 1)).abs())
    T = 2.0 * dinv64.view(-1, 1) * mag + z64.abs() + b.double().abs()
    m = torch.bincount(ei[1][keep], minlength=n).double().view(-1, 1)
    D = float(out_terms(ei, n).max())
    bound = (m + 2 * D + 22) * U * T + ACT_ULPS * U * ref.abs()
    err = (h.cpu().double() - ref).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
    # the rows the formula singles out: above n_P act(b) exactly, an isolated node below it (1 - delta) z + b
    want_top = R.ACTS[act](b)
    torch.testing.assert_close(h[3013:].cpu(), want_top.expand(2, C), rtol=0, atol=ACT_ULPS * U)
    assert torch.equal(h[3013], h[3014])
    torch.testing.assert_close(h[1].cpu(), R.ACTS[act](-z[1] + b), rtol=0, atol=ACT_ULPS * U * 4)
    torch.testing.assert_close(h[6].cpu(), R.ACTS[act](-z[6] + b), rtol=0, atol=ACT_ULPS * U * 4)  # self-loops only


@pytest.mark.parametrize("C", [1, 5, 32, 33, 64])
def test_layer_kernel_has_the_same_bits_on_both_index_routes_and_projects_its_own_rows(C):
    """The list sorted by destination (offsets only) and the shuffled one (permutation) give identical bits: the stable
    sort keeps the edges of every destination in the shuffled list's order (both runs read the same dinv and the same
    coefficient per edge).  The fused projection is h W^T of the rows the launch wrote: C products and C additions per
    entry -> (C + 1) u sum |h| |W|."""
    es, n, z, b = layer_inputs("shuffled", C)
    w = weights(es)
    order = torch.argsort(es[1], stable=True)
    eg = es[:, order].contiguous()
    Cn = (C * 7) % 64 + 1
    wn = torch.randn(Cn, C, generator=torch.Generator().manual_seed(9)).to(dev())
    ds, dst_s, src_s = groups(es, n)
    dg, dst_g, _ = groups(eg, n)
    assert dst_s.perm is not None and dst_g.perm is None
    dinv, coef, _ = K.maxcut_degree(src_s, ds, w.to(dev()))
    zd, bd = z.to(dev()), b.to(dev())
    h1, z1 = K.maxcut_layer(dst_s, ds[0], coef, dinv, zd, bd, K.maxcut_n_p(ds), 1.5, "tanh", wn)
    h2, z2 = K.maxcut_layer(dst_g, dg[0], coef[order.to(dev())].contiguous(), dinv, zd, bd, K.maxcut_n_p(dg), 1.5, "tanh",
                            wn)
    assert torch.equal(h1, h2) and torch.equal(z1, z2) and z1.shape == (n, Cn)
    h64 = h1.cpu().double()
    err = (z1.cpu().double() - h64 @ wn.cpu().double().t()).abs()
    assert bool((err <= (C + 1) * U * (h64.abs() @ wn.cpu().double().abs().t())).all())
    none, z3 = K.maxcut_layer(dst_s, ds[0], coef, dinv, zd, bd, K.maxcut_n_p(ds), 1.5, "tanh", wn, want_h=False)
    assert none is None and torch.equal(z3, z1)


def test_layer_kernel_without_edges_and_with_self_loops_only():
    n, C = 7, 5
    z = torch.randn(n, C, generator=torch.Generator().manual_seed(2)).to(dev())
    b = torch.full((C,), 0.25, device=dev())
    for ei in (torch.zeros(2, 0, dtype=torch.long), torch.tensor([[0, 3, 3], [0, 3, 3]])):
        d, by_dst, by_src = groups(ei, n)
        dinv, coef, _ = K.maxcut_degree(by_src, d, None)
        assert float(dinv.abs().max()) == 0.0
        n_p = K.maxcut_n_p(d)
        h, _ = K.maxcut_layer(by_dst, d[0], coef, dinv, z, b, n_p, 2.0, "identity")
        top = int(n_p)
        assert top == (4 if ei.numel() else 0)
        assert torch.equal(h[top:], b.expand(n - top, C)) and torch.equal(h[:top], -z[:top] + b)


# ------------------------------------------------------------------------------------------------ the row tail
def mlp_bound(v, layers, mlp_act, act):
    """(float64 result, bound) of Linear + act chains on fp32 inputs: a layer's error is |W| e_in (the activations are
    1-Lipschitz) + (in + 2) u (|W| |v| + |b|) for its products, additions and bias + ACT_ULPS u |out|."""
    e = torch.zeros_like(v)
    for k, (wt, b) in enumerate(layers):
        a = mlp_act if k < len(layers) - 1 else act
        pre = v @ wt.t() + b
        e = e @ wt.abs().t() + (wt.size(1) + 2) * U * (v.abs() @ wt.abs().t() + b.abs())
        v = R.ACTS[a](pre)
        e = e + ACT_ULPS * U * v.abs()
    return v, e


@pytest.mark.parametrize("C,units,mlp_act,act", [(8, [16, 16], "relu", "tanh"), (1, [], "relu", "identity"),
                                                 (33, [64, 5, 1], "tanh", "relu"), (64, [3], "identity", "tanh")])
def test_tail_kernel_against_float64(C, units, mlp_act, act):
    g = torch.Generator().manual_seed(17)
    n = 1027  # not a multiple of the four rows of a workgroup
    h = torch.randn(n, C, generator=g)
    dims = [C] + units + [1]
    layers = [(torch.randn(o, i, generator=g) / i ** 0.5, torch.randn(o, generator=g) * 0.3)
              for i, o in zip(dims[:-1], dims[1:])]
    got = K.maxcut_tail(h.to(dev()), [wt.to(dev()) for wt, _ in layers], [b.to(dev()) for _, b in layers], mlp_act, act)
    want, bound = mlp_bound(h.double(), [(wt.double(), b.double()) for wt, b in layers], mlp_act, act)
    err = (got.cpu().double() - want.view(-1)).abs()
    assert got.shape == (n,) and bool((err <= bound.view(-1)).all()), float((err / bound.view(-1)).max())


# ------------------------------------------------------------------------------------------------ the weight gradient
@pytest.mark.parametrize("n,Ca,Cb", [(2500, 5, 33), (1024, 64, 64), (1, 1, 1), (3, 16, 8)])
def test_wgrad_kernel_against_float64(n, Ca, Cb):
    """Each entry: chunks of up to 1024 products added in order, then the chunk sums in order ->
    (1024 + chunks + 1) u sum |a| |b| at the most."""
    g = torch.Generator().manual_seed(23)
    a, b = torch.randn(n, Ca, generator=g), torch.randn(n, Cb, generator=g)
    got = K.maxcut_wgrad(a.to(dev()), b.to(dev()))
    want = a.double().t() @ b.double()
    bound = (min(n, 1024) + (n + 1023) // 1024 + 1) * U * (a.double().abs().t() @ b.double().abs())
    assert got.shape == (Ca, Cb) and bool(((got.cpu().double() - want).abs() <= bound).all())
    assert torch.equal(got, K.maxcut_wgrad(a.to(dev()), b.to(dev())))


# ------------------------------------------------------------------------------------------------ the cut loss
@pytest.mark.parametrize("kind", ["shuffled", "flipped"])
def test_cut_kernel_and_loss_against_float64(kind):
    """(``flipped``: the by-source groups have the lengths 0, 1, 63, 64, 65 and 3000, ``shuffled``: the by-destination
    ones.)  az_i: m_i products added over 64 lanes and folded -> (m_i + 7) u sum |w s|; cut one product more; wsum (m_i + 6) u
    sum |w|.  The loss: per graph the node terms are added in order (n_g terms), divided by a volume with the same kind
    of sum, and averaged over B graphs -> u (2 (n_max + D + 8) + B + 2) mean_g(A_g / vol_g), A_g = sum |w s_src s_dst|."""
    ei, n = graph(kind)
    w = weights(ei)
    s = torch.tanh(torch.randn(n, generator=torch.Generator().manual_seed(31)))
    d, by_dst, by_src = groups(ei, n)
    az, cut, wsum = K.maxcut_cut(by_src, d[1], s.to(dev()), w.to(dev()))
    w64, s64 = w.double(), s.double()
    az64 = torch.zeros(n, dtype=torch.float64).index_add(0, ei[0], w64 * s64[ei[1]])
    mag = torch.zeros(n, dtype=torch.float64).index_add(0, ei[0], (w64 * s64[ei[1]]).abs())
    m = torch.bincount(ei[0], minlength=n).double()
    assert bool(((az.cpu().double() - az64).abs() <= (m + 7) * U * mag).all())
    assert bool(((cut.cpu().double() - s64 * az64).abs() <= (m + 8) * U * mag * s64.abs()).all())
    ws64 = torch.zeros(n, dtype=torch.float64).index_add(0, ei[0], w64)
    assert bool(((wsum.cpu().double() - ws64).abs() <= (m + 6) * U * ws64).all())
    at = K.maxcut_cut(by_dst, d[0], s.to(dev()), w.to(dev()), want_cut=False, want_wsum=False)
    assert at[1] is None and at[2] is None
    at64 = torch.zeros(n, dtype=torch.float64).index_add(0, ei[1], w64 * s64[ei[0]])
    mag_t = torch.zeros(n, dtype=torch.float64).index_add(0, ei[1], (w64 * s64[ei[0]]).abs())
    mt = torch.bincount(ei[1], minlength=n).double()
    assert bool(((at[0].cpu().double() - at64).abs() <= (mt + 7) * U * mag_t).all())
    # the whole loss on a batch cut out of the same list: 5 "graphs" of 603 nodes, the edges between them dropped
    batch = torch.arange(n) // 603
    inside = batch[ei[0]] == batch[ei[1]]
    eb, wb = ei[:, inside].contiguous(), w[inside].contiguous()
    with Routes() as r:
        got = maxcut_loss(s.to(dev()), eb.to(dev()), wb.to(dev()), batch.to(dev()))
    assert r.loss == 1
    want = R.cut_loss(s64, eb, wb.double(), batch)
    A = torch.zeros(5, dtype=torch.float64).index_add(0, batch[eb[0]], (wb.double() * s64[eb[0]] * s64[eb[1]]).abs())
    vol = torch.zeros(5, dtype=torch.float64).index_add(0, batch[eb[0]], wb.double())
    D = float(torch.bincount(eb[0], minlength=n).max())
    bound = U * (2 * (603 + D + 8) + 5 + 2) * float((A / vol).mean())
    assert abs(float(got) - float(want)) <= bound, (float(got), float(want), bound)


@pytest.mark.parametrize("by_destination", [False, True], ids=["by_source", "by_destination"])
def test_cut_kernel_has_the_same_bits_on_both_index_routes(by_destination):
    """The shuffled list (permutation route) against its own stable sort by the grouped row (offsets only)."""
    eh, n = graph("flipped" if not by_destination else "shuffled")  # the long groups on the grouped side
    w = weights(eh)
    s = torch.tanh(torch.randn(n, generator=torch.Generator().manual_seed(31))).to(dev())
    end = 1 if by_destination else 0
    order = torch.argsort(eh[end], stable=True)
    eg = eh[:, order].contiguous()
    outs = []
    for ei, ew in ((eh, w), (eg, w[order].contiguous())):
        d = ei.to(dev())
        grp = K.sag_edge_group(d, n, by_destination=by_destination)
        assert (grp.perm is None) == (ei is eg) and grp.max_members == 3000
        outs.append(K.maxcut_cut(grp, d[1 - end], s, ew.to(dev())))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ------------------------------------------------------------------------------------------------ assignment rounds
def composed_labels(kept, ei, n, rounds):
    labels = torch.zeros(n, dtype=torch.long, device=ei.device)
    labels[kept] = torch.arange(1, kept.numel() + 1, device=ei.device)
    mask = labels > 0
    for _ in range(rounds):
        labels, _, mask = O.propagate_assignments_sparse(labels, ei, kept, mask, kept.numel())
    return labels


def native_labels(kept, ei, n, rounds):
    labels = torch.zeros(n, dtype=torch.int32, device=ei.device)
    labels[kept] = torch.arange(1, kept.numel() + 1, dtype=torch.int32, device=ei.device)
    return K.maxcut_assign_rounds(K.sag_edge_group(ei, n, by_destination=True), ei[0].contiguous(), labels, rounds).long()


def selection(kept, n):
    return SelectOutput(node_index=kept, num_nodes=n, cluster_index=torch.arange(kept.numel(), device=kept.device),
                        num_supernodes=kept.numel())


ROUND_CASES = {
    # name: (kept, edges src -> dst, n, the labels one round must give)
    "tie_lower_label_wins": ([0, 1], [[1, 0], [2, 2]], 3, [1, 2, 1]),
    "duplicates_decide": ([0, 1], [[0, 1, 1], [2, 2, 2]], 3, [1, 2, 2]),
    "chain_one_hop_per_round": ([0], [[0, 1], [1, 2]], 3, [1, 1, 0]),
    "self_loop_and_unlabelled_sources": ([3], [[1, 2, 3, 1], [1, 1, 2, 2]], 4, [0, 0, 1, 1]),
}


@pytest.mark.parametrize("name", sorted(ROUND_CASES))
def test_one_assignment_round(name):
    kept, edges, n, want = ROUND_CASES[name]
    kept, ei = torch.tensor(kept, device=dev()), torch.tensor(edges, device=dev())
    got = native_labels(kept, ei, n, 1)
    assert got.tolist() == want
    assert torch.equal(got, composed_labels(kept, ei, n, 1))


def test_a_vote_that_interleaves_across_the_lanes_of_the_walk():
    """130 edges into one node from three kept nodes, their labels cycling 1, 2, 3, 1, ... through the group: counts
    43 / 44 / 43, so no 64-lane chunk of the walk sees the winner alone."""
    kept = torch.tensor([0, 1, 2], device=dev())
    src = torch.tensor([0, 1, 2], device=dev()).repeat(44)[:130]
    src[129] = 1  # 0: 43, 1: 44, 2: 43
    ei = torch.stack([src, torch.full_like(src, 3)])
    assert torch.bincount(src).tolist() == [43, 44, 43]
    got = native_labels(kept, ei, 4, 1)
    assert got.tolist() == [1, 2, 3, 2]
    assert torch.equal(got, composed_labels(kept, ei, 4, 1))


@pytest.mark.parametrize("kind", ["sorted", "shuffled"])
def test_assignment_rounds_match_the_composed_routine_on_the_hub_graph(kind):
    ei, n = graph(kind)
    d = ei.to(dev())
    kept = torch.arange(10, 3013, 5, device=dev())
    for rounds in (1, 3):
        assert torch.equal(native_labels(kept, d, n, rounds), composed_labels(kept, d, n, rounds))
    # the whole routine: labels, leftovers inside their graph (one graph here), the relabelling
    sel = MaxCutSelect(4, mp_units=[4], mlp_units=[])
    so = selection(kept, n)
    batch = torch.zeros(n, dtype=torch.long, device=dev())
    with Routes() as r:
        got = sel.assign(so, d, None, batch, 3)
    assert r.rounds == 1 and got.num_supernodes == kept.numel() and got.node_index.numel() == n
    reached = composed_labels(kept, d, n, 3)
    ok = reached > 0
    assert 0 < int((~ok).sum()) < n  # nodes 1 and 6 and the two above n_P have no in-edge from another node
    assert torch.equal(got.cluster_index[ok], reached[ok] - 1)


def test_a_list_with_a_longer_group_than_the_rounds_take_goes_to_the_composed_routine(monkeypatch):
    ei, n = graph("shuffled")
    d = ei.to(dev())
    kept = torch.arange(10, 3013, 5, device=dev())
    sel = MaxCutSelect(4, mp_units=[4], mlp_units=[])
    batch = torch.zeros(n, dtype=torch.long, device=dev())
    assert K.MAXCUT_ASSIGN_MAX_GROUP == 4096 and K.sag_edge_group(d, n).max_members == 3000
    with Routes() as r:
        native = sel.assign(selection(kept, n), d, None, batch, 3)
    assert r.rounds == 1
    monkeypatch.setattr(K, "MAXCUT_ASSIGN_MAX_GROUP", 2999)
    with Routes() as r:
        composed = sel.assign(selection(kept, n), d, None, batch, 3)
    assert r.rounds == 0
    ok = composed_labels(kept, d, n, 3) > 0
    assert torch.equal(native.cluster_index[ok], composed.cluster_index[ok])


def test_chains_longer_than_max_iter_leave_their_tail_to_the_draw_inside_the_graph():
    c = CASES["maxcut_leftovers"]
    i = c["inputs"]
    p = build(c)
    torch.manual_seed(0)
    with torch.no_grad(), Routes() as r:
        so = p.selector(x=i["x"].to(dev()), edge_index=i["edge_index"].to(dev()), batch=i["batch"].to(dev()))
    assert r.rounds == 1
    kept = torch.sort(c["expected"]["kept"])[0]
    want = torch.tensor(R.assign_rounds(kept, i["edge_index"], i["x"].size(0), c["cfg"]["max_iter"]))
    reached = want > 0
    ci = so.cluster_index.cpu()
    assert 0 < int(reached.sum()) < want.numel() and so.num_supernodes == kept.numel()
    assert torch.equal(ci[reached], want[reached] - 1)
    assert torch.equal(i["batch"][kept[ci]], i["batch"])


def test_a_batch_where_every_node_is_kept():
    c = CASES["maxcut_weighted"]
    cfg = dict(c["cfg"], ratio=0.999)
    p = MaxCutPooling(**cfg).eval()
    p.load_state_dict(c["params"])
    p = p.to(dev())
    with torch.no_grad(), Routes() as r:
        out = forward(p, c)
    n = c["inputs"]["x"].size(0)
    assert r.rounds == 0 and out.so.num_supernodes == n and out.x.shape == (n, 4)
    assert torch.equal(torch.sort(out.so.node_index)[0].cpu(), torch.arange(n))


# ------------------------------------------------------------------------------------------------ determinism
def test_two_training_calls_give_identical_bits():
    c = CASES["maxcut_12_layers"]
    runs = []
    for _ in range(2):
        p = build(c, requires_grad=True)
        x = c["inputs"]["x"].to(dev()).requires_grad_(True)
        out = forward(p, c, x=x)
        ((out.x ** 2).sum() + out.loss["maxcut_loss"]).backward()
        runs.append([out.x.detach(), out.so.scores.detach(), out.loss["maxcut_loss"].detach(), out.edge_weight.detach(),
                     x.grad] + [q.grad for q in p.parameters()])
    assert all(g is not None for g in runs[0])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    ei, n = graph("shuffled")  # and on the graph with the long group, widths 32 -> 16
    net = MaxCutScoreNet(6, mp_units=[32, 16], mlp_units=[8]).to(dev())
    x0 = torch.randn(n, 6, generator=torch.Generator().manual_seed(1))
    d, w = ei.to(dev()), weights(ei).to(dev())
    runs = []
    for _ in range(2):
        net.zero_grad()
        x = x0.to(dev()).requires_grad_(True)
        s = net(x, d, w)
        (s.view(-1) * torch.linspace(-1, 1, n, device=dev())).sum().backward()
        runs.append([s.detach(), x.grad] + [q.grad.clone() for q in net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("name", ["maxcut_default", "maxcut_weighted", "maxcut_loops_duplicates", "maxcut_isolated",
                                  "maxcut_12_layers", "maxcut_delta", "maxcut_identity_acts", "maxcut_relu_layers",
                                  "maxcut_no_assign_all"])
def test_gradients_of_the_pooler_by_path_against_the_float64_restatement(name):
    """sum(x_pool^2) alone and the loss alone through the whole public class: x and every parameter against the float64
    restatement, with its float32 run as the measure.  (The fixture stores the gradients of the SUM of the two paths;
    test_maxcut_restatement.py pins the restatement to them at 1e-11, and the test below compares the product with the
    stored numbers directly.)"""
    c = CASES[name]
    names = sorted(c["params"])
    kept = c["expected"]["kept"]

    def kernel():
        p = build(c, requires_grad=True)
        x = c["inputs"]["x"].to(dev()).requires_grad_(True)
        with Routes() as r:
            out = forward(p, c, x=x)
        assert r.score == 1 and r.loss == 1
        assert torch.equal(out.so.cluster_index.cpu(), c["expected"]["so"]["cluster_index"])
        return ({"sum_sq": (out.x ** 2).sum(), "loss": out.loss["maxcut_loss"]},
                {"x": x, **dict(p.named_parameters())})

    def oracle(dtype):
        par = {k: v.to(dtype).requires_grad_(True) for k, v in c["params"].items()}
        x = c["inputs"]["x"].to(dtype).requires_grad_(True)
        got = R.pool_case(c, dtype, collapsed=False, params=par, x=x, kept=kept)
        return {"sum_sq": (got["x_pool"] ** 2).sum(), "loss": got["loss"]}, {"x": x, **par}

    check_grad_paths(name, kernel, oracle, ["x"] + names)


@pytest.mark.parametrize("name", POOL)
def test_gradients_of_the_fixtures_objective_match_the_stored_float64_gradients(name):
    """The fixture's own objective, sum(x_pool^2) + loss, against the gradients the reference's float64 run stored.  The
    bound is the project's float32 tolerance taken normwise: ||G - G_64|| <= 1e-5 ||G_64|| for x and for all parameters
    together (the by-path test above holds each leaf to a multiple of ATen's own float32 error, which is tighter)."""
    c = CASES[name]
    f = c["f64"]["grads"]
    p = build(c, requires_grad=True)
    x = c["inputs"]["x"].to(dev()).requires_grad_(True)
    out = forward(p, c, x=x)
    par = dict(p.named_parameters())
    grads = torch.autograd.grad((out.x ** 2).sum() + out.loss["maxcut_loss"], [x] + [par[k] for k in f["names"]],
                                allow_unused=True)
    flat = torch.cat([(torch.zeros_like(par[k]) if g is None else g).reshape(-1) for k, g in zip(f["names"], grads[1:])])
    for got, want in ((grads[0], f["x"]), (flat, f["params_flat"])):
        err = float(torch.linalg.vector_norm(got.cpu().double() - want)) / float(torch.linalg.vector_norm(want))
        print(f"{name}: normwise error {err:.2e}")
        assert err <= 1e-5


def test_gradients_of_the_score_net_on_the_hub_graph():
    ei, n = graph("shuffled")
    w0 = weights(ei)
    x0 = torch.randn(n, 6, generator=torch.Generator().manual_seed(7))
    torch.manual_seed(3)
    ref = MaxCutPooling(6, mp_units=[33, 16, 5], mlp_units=[8])
    with torch.no_grad():
        for q in ref.parameters():
            if q.dim() == 1:
                q.uniform_(-0.5, 0.5)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    cfg = dict(mp_units=[33, 16, 5], mlp_units=[8])
    names = sorted(state)

    def kernel():
        p = MaxCutPooling(6, **cfg)
        p.load_state_dict(state)
        p = p.to(dev())
        x = x0.to(dev()).requires_grad_(True)
        with Routes() as r:
            s = p.selector.score_net(x, ei.to(dev()), w0.to(dev())).view(-1)
        assert r.score == 1
        return {"scores": s}, {"x": x, **dict(p.named_parameters())}

    def oracle(dtype):
        par = {k: v.to(dtype).requires_grad_(True) for k, v in state.items()}
        x = x0.to(dtype).requires_grad_(True)
        return {"scores": R.scores_reference_shaped(par, cfg, x, ei, w0.to(dtype))}, {"x": x, **par}

    check_grad_paths("maxcut/hub", kernel, oracle, ["x"] + names)


# ------------------------------------------------------------------------------------------------ memory
def test_the_score_net_takes_nothing_of_size_e_times_c():
    """A warm no-grad call at N = 4096, E = 262144, F = 32 may raise the peak by a quarter of one E x 32 float matrix
    (8.4 MB) at the most; its own buffers are two N x 32 planes, E coefficients and a few N-vectors, about 3 MB."""
    n, E, F = 4096, 262144, 32
    g = torch.Generator().manual_seed(11)
    ei = torch.randint(0, n, (2, E), generator=g).to(dev())
    x = torch.randn(n, F, generator=g).to(dev())
    net = MaxCutScoreNet(F, mp_units=[32, 32, 32, 32]).to(dev())
    with torch.no_grad():
        warm = net(x, ei)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with Routes() as r:
            again = net(x, ei)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    print(f"score net: peak rise {rise} bytes (E*32*4 = {E * 32 * 4})")
    assert r.score == 1 and torch.equal(warm, again)
    assert rise < E * 32 * 4 // 4


# ------------------------------------------------------------------------------------------------ non-finite inputs
@pytest.mark.parametrize("what", ["nan_row", "inf_weight", "negative_degree"])
def test_non_finite_inputs_follow_the_composed_device_form(what):
    c = CASES["maxcut_directed_weighted"]
    i = c["inputs"]
    x, ew = i["x"].clone(), i["edge_weight"].clone()
    if what == "nan_row":
        x[3] = float("nan")
    elif what == "inf_weight":
        ew[5] = float("inf")
    else:
        ew[i["edge_index"][0] == int(i["edge_index"][0, 0])] = -1.0  # one node's out-degree goes below zero
    net = build(c).selector.score_net
    args = (x.to(dev()), i["edge_index"].to(dev()), ew.to(dev()))
    with torch.no_grad():
        with Routes() as r:
            got = net(*args).view(-1)
        assert r.score == 1
        net.native_case = lambda *a: False
        with Routes() as r:
            want = net(*args).view(-1)
        assert r.score == 0
        loss_got = maxcut_loss(got, args[1], args[2], i["batch"].to(dev()))
    assert bool(torch.isnan(want).any()) and not bool(torch.isnan(want).all())
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and torch.equal(got[torch.isinf(got)], want[torch.isinf(want)])
    fin = torch.isfinite(want)
    torch.testing.assert_close(got[fin], want[fin], rtol=1e-5, atol=1e-5)
    assert bool(torch.isnan(loss_got))  # a NaN score reaches the loss of its graph and the mean


# ------------------------------------------------------------------------------------------------ routing
def test_which_inputs_take_the_native_route():
    c = CASES["maxcut_weighted"]
    i = c["inputs"]
    d = dev()
    x, ei, ew, batch = i["x"].to(d), i["edge_index"].to(d), i["edge_weight"].to(d), i["batch"].to(d)
    p = build(c)
    with torch.no_grad():
        with Routes() as r:
            base = p(x=x, adj=ei, edge_weight=ew, batch=batch)
        assert (r.score, r.loss, r.rounds) == (1, 1, 1)
        with Routes() as r:  # float64: composed score net and loss; the integer rounds do not care
            p64 = build(c, dtype=torch.float64)
            out = p64(x=x.double(), adj=ei, edge_weight=ew.double(), batch=batch)
        assert (r.score, r.loss) == (0, 0)
        torch.testing.assert_close(out.so.scores.float(), base.so.scores, rtol=1e-5, atol=1e-5)
        assert torch.equal(out.so.cluster_index, base.so.cluster_index)
        with Routes() as r:  # sparse connectivity: composed
            coo = torch.sparse_coo_tensor(ei, ew, (x.size(0), x.size(0))).coalesce()
            s = p.selector.score_net(x, coo)
        assert r.score == 0
        want = p.selector.score_net(x, coo.indices(), coo.values())
        torch.testing.assert_close(s, want, rtol=1e-5, atol=1e-5)
        wide = MaxCutScoreNet(4, mp_units=[65, 8], mlp_units=[4]).to(d)  # a width of 65: composed
        narrow = MaxCutScoreNet(4, mp_units=[64, 8], mlp_units=[4]).to(d)
        with Routes() as r:
            wide(x, ei, ew)
            assert r.score == 0
            narrow(x, ei, ew)
            assert r.score == 1
    with Routes() as r:  # an edge weight that asks for a gradient: composed, and it gets one
        ewg = ew.clone().requires_grad_(True)
        out = p(x=x, adj=ei, edge_weight=ewg, batch=batch)
        (out.loss["maxcut_loss"] + out.so.scores.sum()).backward()
    assert (r.score, r.loss) == (0, 0) and ewg.grad is not None and bool(ewg.grad.abs().sum() > 0)
    torch.testing.assert_close(out.so.scores.detach(), base.so.scores, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kind", ["shuffled", "flipped"])
def test_a_list_with_a_hub_sends_the_score_net_to_the_composed_form(kind, monkeypatch):
    """The gate reads the longest group of both indices (the forward walks by destination, the backward by source)."""
    ei, n = graph(kind)
    d, w = ei.to(dev()), weights(ei).to(dev())
    x = torch.randn(n, 6, generator=torch.Generator().manual_seed(1)).to(dev())
    net = MaxCutScoreNet(6, mp_units=[16, 8], mlp_units=[8]).to(dev())
    assert (K.MAXCUT_SCORE_MAX_GROUP, K.MAXCUT_SCORE_GROUP_SHARE) == (4096, 256) and not K.maxcut_score_has_hub(d, n)
    with torch.no_grad():
        with Routes() as r:
            native = net(x, d, w)
        assert r.score == 1
        monkeypatch.setattr(K, "MAXCUT_SCORE_MAX_GROUP", 2999)
        assert K.maxcut_score_has_hub(d, n)
        with Routes() as r:
            composed = net(x, d, w)
        assert r.score == 0
        monkeypatch.setattr(K, "MAXCUT_SCORE_MAX_GROUP", 16)  # E / 256 = 47 is the larger bound now: still a hub
        assert K.maxcut_score_has_hub(d, n)
        monkeypatch.setattr(K, "MAXCUT_SCORE_GROUP_SHARE", 4)  # E / 4 = 3 052: no hub any more
        assert not K.maxcut_score_has_hub(d, n)
    torch.testing.assert_close(native, composed, rtol=1e-5, atol=1e-5)


def test_the_second_call_hits_the_memos_and_the_score_net_does_not_wait_for_the_device():
    ei, n = graph("shuffled")
    d, w = ei.to(dev()), weights(ei).to(dev())
    x = torch.randn(n, 6, generator=torch.Generator().manual_seed(1)).to(dev())
    net = MaxCutScoreNet(6, mp_units=[16, 8], mlp_units=[8]).to(dev())
    with torch.no_grad():
        first = net(x, d, w)
        memo = K._SAG_GROUPS.get(d)
        assert sorted(memo) == [(n, False), (n, True)]
        by_dst, by_src, n_p = memo[(n, True)], memo[(n, False)], K._MAXCUT_NP.get(d)
        assert n_p is not None and int(n_p) == 3013
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                second = net(x, d, w)
            finally:
                torch.cuda.set_sync_debug_mode("default")
    waits = [str(m.message) for m in seen if "called a synchronizing" in str(m.message)]
    assert not waits, waits
    assert torch.equal(first, second)
    memo = K._SAG_GROUPS.get(d)
    assert memo[(n, True)] is by_dst and memo[(n, False)] is by_src and K._MAXCUT_NP.get(d) is n_p
    d.add_(0)  # an in-place write moves the version: the facts of the old contents are not used
    assert K._SAG_GROUPS.get(d) is None and K._MAXCUT_NP.get(d) is None
