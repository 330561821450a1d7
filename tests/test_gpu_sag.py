"""SAGPooling on the MI355X: the public class against the reference's stored results, the two scorer kernels against
float64 with bounds derived from the arithmetic (never tuned), run-to-run determinism, gradients one upstream path at a
time at fp32's own error (the helper of test_gpu_grad_paths.py), and the memory the scorer may not take: nothing of size
E x F.  Without the native scorer this module fails at import; a composed fallback on the device would fail the memory
test and, on the hub graph, the per-node bounds of a sum taken in another order are not what is asserted -- the parity
and memory tests are the ones that pin the path."""
import os

import pytest
import torch

import sag_restatement as R
from test_gpu_grad_paths import check_grad_paths

from tgp import functions as Fn
from tgp import kernels as K
from tgp.poolers import SAGPooling

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_sag_v1.pt"), weights_only=True)["cases"]
U = 2.0 ** -24  # fp32 unit roundoff


def dev():
    return torch.device("cuda:0")


def build(c, requires_grad=False):
    p = SAGPooling(GNN=c["gnn"], **c["cfg"]).eval()
    p.load_state_dict(c["params"])
    p = p.to(dev())
    for q in p.parameters():
        q.requires_grad_(requires_grad)
    return p


def forward(p, c, x=None):
    i = c["inputs"]
    d = dev()
    mv = lambda t: None if t is None else t.to(d)  # noqa: E731
    return p(x=mv(i["x"]) if x is None else x, adj=mv(i["edge_index"]), edge_weight=mv(i["edge_weight"]),
             batch=mv(i["batch"]), attn=mv(i.get("attn")))


# ------------------------------------------------------------------------------------------------ the public class
@pytest.mark.parametrize("grad", [False, True], ids=["no_grad", "grad"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_parity_through_the_public_class(name, grad):
    c = CASES[name]
    e = c["expected"]
    p = build(c, requires_grad=grad)
    with torch.set_grad_enabled(grad):
        out = forward(p, c)
    so = out.so
    assert out.x.requires_grad == grad and so.weight.requires_grad == grad
    assert torch.equal(so.node_index.cpu(), e["so"]["node_index"]), name
    assert torch.equal(so.cluster_index.cpu(), e["so"]["cluster_index"]), name
    assert so.num_nodes == e["so"]["num_nodes"] and so.num_supernodes == e["so"]["num_supernodes"]
    assert torch.equal(out.edge_index.cpu(), e["edge_index"]), name
    if e["batch"] is None:
        assert out.batch is None
    else:
        assert torch.equal(out.batch.cpu(), e["batch"]), name
    torch.testing.assert_close(so.weight.detach().cpu(), e["so"]["weight"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out.x.detach().cpu(), e["x"], rtol=1e-5, atol=1e-5)
    if e["edge_weight"] is None:
        assert out.edge_weight is None
    else:
        torch.testing.assert_close(out.edge_weight.detach().cpu(), e["edge_weight"], rtol=1e-5, atol=1e-5)


def test_the_layers_return_the_raw_column_on_the_device():
    for name in ("sag_graphconv_mean", "sag_sage_directed", "sag_attn_1d"):
        c = CASES[name]
        p = build(c)
        i = c["inputs"]
        a = i["x"] if i.get("attn") is None else i["attn"]
        with torch.no_grad():
            raw = p.gnn(a.to(dev()), i["edge_index"].to(dev()))
        assert raw.shape == (a.size(0), 1) and raw.is_cuda
        torch.testing.assert_close(raw.view(-1).cpu(), c["expected"]["score"], rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ row_project2
def _project_case(n, f, strided):
    g = torch.Generator().manual_seed(1000 * n + 10 * f + len(str(strided)))
    if strided == "unaligned":  # a column slice: row stride f + 3, base 4 bytes past a 16-byte boundary
        x = torch.randn(n, f + 3, generator=g).to(dev())[:, 1:1 + f]
        assert x.stride(0) == f + 3 and x.data_ptr() % 16 != 0
    elif strided == "aligned":  # a column slice that keeps the 16-byte loads: row stride a multiple of 4, base aligned
        x = torch.randn(n, (f + 7) // 4 * 4, generator=g).to(dev())[:, :f]
        assert x.stride(0) % 4 == 0 and x.stride(0) > f and x.data_ptr() % 16 == 0
    else:
        x = torch.randn(n, f, generator=g).to(dev())
    return x, torch.randn(f, generator=g).to(dev()), torch.randn(1, f, generator=g).to(dev())


@pytest.mark.parametrize("strided", [False, "unaligned", "aligned"], ids=["contiguous", "slice_unaligned", "slice_aligned"])
@pytest.mark.parametrize("f", [1, 3, 4, 5, 64, 67, 130])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_row_project2_against_float64(n, f, strided):
    """Per row |out - <x, w>_64| <= (F + 2) 2^-24 sum_f |x_f w_f|: F products and F - 1 additions in any order cost at
    most (F + 1) roundings of partial sums no larger than sum |x_f w_f| (fused or not), one more for the lane fold."""
    x, w0, w1 = _project_case(n, f, strided)
    p, q = K.row_project2(x, w0, w1)
    assert p.shape == (n,) and q.shape == (n,)
    x64 = x.double().cpu()
    for got, w in ((p, w0), (q, w1)):
        w64 = w.double().cpu().view(-1)
        want = x64 @ w64
        bound = (f + 2) * U * (x64.abs() @ w64.abs())
        err = (got.double().cpu() - want).abs()
        print(f"row_project2 n={n} f={f} {strided}: max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all())


def test_row_project2_very_wide_rows():
    """Beyond the eight register chunks of a lane (F > 64 * 4 * 8 with 16-byte loads, F > 64 * 8 without)."""
    for f, strided in ((2052, False), (2053, "aligned"), (515, False)):
        x, w0, w1 = _project_case(3, f, strided)
        p, q = K.row_project2(x, w0, w1)
        x64 = x.double().cpu()
        for got, w in ((p, w0), (q, w1)):
            w64 = w.double().cpu().view(-1)
            assert bool(((got.double().cpu() - x64 @ w64).abs() <= (f + 2) * U * (x64.abs() @ w64.abs())).all())


# ------------------------------------------------------------------------------------------------ the aggregate
N_HUB, HUB, HUB_DEG = 4000, 7, 3000
_hub_memo = {}


def hub_graph():
    """Host edge lists of one graph of 4000 nodes: 9000 random edges among the first 3900 nodes (the last 100 have no
    incoming and no outgoing edge; some of the others have no incoming edge either), 300 of them listed twice, 150
    self-loops and one hub of in-degree 3000.  ``grouped``: stably sorted by destination (offsets-only route);
    ``shuffled``: the same edges in random order (permutation route)."""
    if not _hub_memo:
        g = torch.Generator().manual_seed(77)
        ei = torch.randint(0, N_HUB - 100, (2, 9000), generator=g)
        loops = torch.randperm(N_HUB - 100, generator=g)[:150]
        hub = torch.stack([torch.randint(0, N_HUB - 100, (HUB_DEG,), generator=g), torch.full((HUB_DEG,), HUB)])
        ei = torch.cat([ei, ei[:, :300], torch.stack([loops, loops]), hub], 1)
        grouped = ei[:, torch.argsort(ei[1], stable=True)].contiguous()
        shuffled = ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()
        indeg = torch.bincount(ei[1], minlength=N_HUB)
        assert int(indeg[HUB]) >= HUB_DEG and int((indeg == 0).sum()) >= 100
        assert bool((grouped[1][1:] >= grouped[1][:-1]).all()) and not bool((shuffled[1][1:] >= shuffled[1][:-1]).all())
        _hub_memo.update(grouped=grouped, shuffled=shuffled, indeg=indeg)
    return _hub_memo


def _aggregate_reference(ei, p, q, b, mean):
    n = p.numel()
    p64, q64 = p.double().cpu(), q.double().cpu()
    s = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], p64[ei[0]])
    mag = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], p64[ei[0]].abs())
    indeg = torch.bincount(ei[1], minlength=n)
    if mean:
        s, mag = s / indeg.clamp(min=1), mag / indeg.clamp(min=1)
    return s + b + q64, (indeg + 3) * U * (q64.abs() + abs(b) + mag), indeg


@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("layout", ["grouped", "shuffled"])
def test_aggregate_against_float64(layout, mean):
    """|t - t_64| <= (indeg + 3) 2^-24 (|q| + |b| + sum |p_src|): indeg - 1 additions inside the group, the bias, the
    root term and the division of the mean, each one rounding of a partial sum no larger than the sum of magnitudes."""
    h = hub_graph()
    ei = h[layout]
    g = torch.Generator().manual_seed(5)
    p, q = torch.randn(N_HUB, generator=g).to(dev()), torch.randn(N_HUB, generator=g).to(dev())
    bias = torch.tensor([0.37]).to(dev())
    ei_d = ei.to(dev())
    grp = K.sag_edge_group(ei_d, N_HUB, by_destination=True)
    assert (grp.perm is None) == (layout == "grouped")
    t, a = K.sag_aggregate(grp, ei_d[0], p, q, bias, mean=mean, tanh=True, want_t=True)
    want, bound, indeg = _aggregate_reference(ei, p, q, float(bias.double().cpu()), mean)
    err = (t.double().cpu() - want).abs()
    print(f"aggregate {layout} mean={mean}: max err/bound {float((err / bound).max()):.3f}, hub {float(err[HUB] / bound[HUB]):.3f}")
    assert bool((err <= bound).all())
    # a node without an incoming edge is exactly (0 + b) + q
    lone = indeg == 0
    assert torch.equal(t.cpu()[lone], ((torch.zeros_like(q) + bias) + q).cpu()[lone])
    # the fused activation: tanhf of the very t that was written (4 ulp of a value below 1), identity returns t itself
    assert float((a.double().cpu() - torch.tanh(t.double().cpu())).abs().max()) <= 4 * U
    assert torch.equal(K.sag_aggregate(grp, ei_d[0], p, q, bias, mean=mean, tanh=False), t)
    # without root term and bias
    t0 = K.sag_aggregate(grp, ei_d[0], p, None, None, mean=mean)
    want0, bound0, _ = _aggregate_reference(ei, p, torch.zeros_like(q), 0.0, mean)
    assert bool(((t0.double().cpu() - want0).abs() <= bound0).all())


def test_aggregate_without_edges_and_with_sources_out_of_range():
    d = dev()
    p, q = torch.randn(9, device=d), torch.randn(9, device=d)
    bias = torch.tensor([0.5], device=d)
    empty = torch.zeros(2, 0, dtype=torch.long, device=d)
    grp = K.sag_edge_group(empty, 9)
    assert grp.nnz == 0 and grp.perm is None
    assert torch.equal(K.sag_aggregate(grp, empty[0], p, q, bias), (torch.zeros_like(q) + bias) + q)
    x = torch.randn(9, 4, device=d)
    w = torch.randn(1, 4, device=d)
    a = K.sag_score(x, empty, w, w, bias, mean=True, tanh=True)
    torch.testing.assert_close(a, torch.tanh(x @ w.view(-1) + bias), rtol=1e-5, atol=1e-6)
    # a source id outside [0, n) is skipped (never dereferenced); it still counts in the mean's group size
    ei = torch.tensor([[0, 99, 2, -1], [1, 1, 1, 3]], device=d)
    grp = K.sag_edge_group(ei, 9)
    t = K.sag_aggregate(grp, ei[0], p, None, None)
    want = torch.zeros(9, device=d)
    want[1] = p[0] + p[2]
    assert torch.equal(t, want)
    tm = K.sag_aggregate(grp, ei[0], p, None, None, mean=True)
    assert torch.equal(tm[1], (p[0] + p[2]) / 3) and float(tm[3]) == 0.0


@pytest.mark.parametrize("layout", ["grouped", "shuffled"])
def test_the_score_is_bit_identical_run_to_run(layout):
    ei = hub_graph()[layout].to(dev())
    g = torch.Generator().manual_seed(9)
    x = torch.randn(N_HUB, 32, generator=g).to(dev())
    w_rel, w_root = torch.randn(1, 32, generator=g).to(dev()) * 0.05, torch.randn(1, 32, generator=g).to(dev())
    bias = torch.tensor([0.1]).to(dev())
    first = K.sag_score(x, ei, w_rel, w_root, bias, mean=False, tanh=True, want_t=True)
    K._SAG_GROUPS.clear()  # the second call rebuilds its index as well
    second = K.sag_score(x, ei.clone(), w_rel, w_root, bias, mean=False, tanh=True, want_t=True)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    gt = torch.randn(N_HUB, generator=g).to(dev())
    by_src = K.sag_edge_group(ei, N_HUB, by_destination=False)
    assert torch.equal(K.sag_aggregate(by_src, ei[1], gt), K.sag_aggregate(by_src, ei[1], gt))


# ------------------------------------------------------------------------------------------------ backward kernel
@pytest.mark.parametrize("f", [4, 5, 64])
@pytest.mark.parametrize("accumulate", [False, True])
def test_bwd_x_against_float64(f, accumulate):
    """Two products and one addition (two with an incoming gradient): at most 3 (4) roundings of values no larger than
    the sum of the magnitudes."""
    g = torch.Generator().manual_seed(f)
    n = 300
    gq, gp = torch.randn(n, generator=g).to(dev()), torch.randn(n, generator=g).to(dev())
    wr, wl = torch.randn(1, f, generator=g).to(dev()), torch.randn(1, f, generator=g).to(dev())
    old = torch.randn(n, f, generator=g).to(dev())
    got = K.sag_score_bwd_x(gq, gp, wr, wl, old.clone() if accumulate else None)
    a = gq.double().cpu().view(-1, 1) * wr.double().cpu()
    b = gp.double().cpu().view(-1, 1) * wl.double().cpu()
    want, mag = a + b, a.abs() + b.abs()
    if accumulate:
        want, mag = want + old.double().cpu(), mag + old.double().cpu().abs()
    assert bool(((got.double().cpu() - want).abs() <= 4 * U * mag).all())


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("name", ["sag_graphconv_batch", "sag_graphconv_mean", "sag_sage_directed", "sag_identity",
                                  "sag_keep_self_loops", "sag_attn_2d", "sag_multiplier"])
def test_gradients_of_the_pooler_one_path_at_a_time(name):
    """x_pool alone, so.weight alone, and the fixture's objective sum(x_pool^2), against the float64 restatement (which
    tests/test_sag_restatement.py pins to the fixture's float64 gradients at 1e-9) with the restatement in float32 as
    the measure of fp32's own error."""
    c = CASES[name]
    names = sorted(c["params"])
    perm_of = {}

    def kernel():
        p = build(c, requires_grad=True)
        x = c["inputs"]["x"].to(dev()).requires_grad_(True)
        out = forward(p, c, x=x)
        assert out.x.requires_grad and out.so.weight.requires_grad
        perm = torch.empty_like(out.so.node_index)
        perm[out.so.cluster_index] = out.so.node_index
        perm_of["kernel"] = perm.cpu()
        w = torch.zeros_like(out.so.weight).index_put((out.so.cluster_index,), out.so.weight)  # in supernode order
        lv = {"x": x, **{k: dict(p.named_parameters())[k] for k in names}}
        return {"x_pool": out.x, "weight": w, "sum_sq": (out.x ** 2).sum()}, lv

    def oracle(dtype):
        x = c["inputs"]["x"].to(dtype).requires_grad_(True)
        par = {k: v.to(dtype).requires_grad_(True) for k, v in c["params"].items()}
        _, _, perm, weight, x_pool = R.pool_case(c, dtype, params=par, x=x)
        perm_of[dtype] = perm
        return {"x_pool": x_pool, "weight": weight, "sum_sq": (x_pool ** 2).sum()}, {"x": x, **par}

    check_grad_paths(name, kernel, oracle, ["x"] + names)
    assert torch.equal(perm_of["kernel"], perm_of[torch.float64]) and torch.equal(perm_of["kernel"], perm_of[torch.float32])


@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("use_tanh", [True, False], ids=["tanh", "identity"])
@pytest.mark.parametrize("layout", ["grouped", "shuffled"])
def test_gradients_of_the_scorer_on_the_hub_graph(layout, use_tanh, mean):
    """The one autograd node against the float64 restatement on the graph with the in-degree-3000 hub (whose source
    nodes' g_p and whose own g_t take the long sums), both index routes."""
    ei = hub_graph()[layout]
    F = 8
    g = torch.Generator().manual_seed(21)
    x0 = torch.randn(N_HUB, F, generator=g)
    # a neighbour weight small enough that tanh saturates at the hub only
    vals = {"w_rel": torch.randn(1, F, generator=g) * 0.1, "w_root": torch.randn(1, F, generator=g) * 0.5,
            "bias": torch.tensor([0.2])}
    ei_d = ei.to(dev())

    def kernel():
        x = x0.to(dev()).requires_grad_(True)
        lv = {k: v.to(dev()).requires_grad_(True) for k, v in vals.items()}
        a = Fn.sag_score(x, ei_d, lv["w_rel"], lv["w_root"], lv["bias"], mean, use_tanh)
        assert type(a.grad_fn).__name__ == "_SagScoreFnBackward"
        return {"a": a}, {"x": x, **lv}

    def oracle(dtype):
        x = x0.to(dtype).requires_grad_(True)
        lv = {k: v.to(dtype).requires_grad_(True) for k, v in vals.items()}
        t = R.raw_score(x, ei, lv["w_rel"], lv["w_root"], lv["bias"], mean)
        return {"a": torch.tanh(t) if use_tanh else t}, {"x": x, **lv}

    check_grad_paths(f"hub/{layout}/{use_tanh}/{mean}", kernel, oracle, ["x", "w_rel", "w_root", "bias"])


def test_sageconv_without_root_weight_trains():
    """No root term: x gets its gradient through the neighbours alone, and there is no ``lin_r`` to train."""
    from tgp.nn import SAGEConv
    torch.manual_seed(3)
    state = SAGEConv(4, 1, root_weight=False).state_dict()
    ei = hub_graph()["shuffled"][:, :2000]
    x0 = torch.randn(N_HUB, 4, generator=torch.Generator().manual_seed(4))

    def run(device, dtype):
        conv = SAGEConv(4, 1, root_weight=False).to(dtype)
        conv.load_state_dict({k: v.to(dtype) for k, v in state.items()})
        conv = conv.to(device)
        x = x0.to(device, dtype).requires_grad_(True)
        return {"raw": conv(x, ei.to(device))}, {"x": x, **dict(conv.named_parameters())}

    check_grad_paths("sage_no_root", lambda: run(dev(), torch.float32), lambda dtype: run("cpu", dtype),
                     ["x", "lin_l.weight", "lin_l.bias"])


# ------------------------------------------------------------------------------------------------ memory
def test_the_scorer_forms_no_e_by_f_temporary():
    """N = 4096, E = 200 000, F = 64: the composed form gathers an E x F message matrix (51.2 MB).  The native scorer
    allocates its two projections and its output (12 N bytes); the int32 by-destination index (4 N + 4 E bytes) is built
    once per edge list and remembered, so the memo is warmed first and what is measured is the steady-state call."""
    n, E, F = 4096, 200_000, 64
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, F, generator=g).to(dev())
    ei = torch.randint(0, n, (2, E), generator=g).to(dev())
    pool = SAGPooling(F).to(dev()).eval()
    with torch.no_grad():
        warm = pool.gnn.score(x, ei, True)  # builds and remembers the by-destination index
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        a = pool.gnn.score(x, ei, True)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    print(f"scorer call: peak rise {rise} bytes (E*F*4 = {E * F * 4})")
    assert torch.equal(a, warm)
    assert rise < E * F * 4 // 4
