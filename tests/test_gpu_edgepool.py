"""Edge-contraction pooling on the GPU (csrc/edge_contract.hip through tgp.kernels / EdgeContractionSelect /
EdgeContractionPooling).

1. Fixture parity with the reference (tests/golden/golden_edgepool_v1.pt): indices exact, values at rtol = atol = 1e-5.
2. The matching with an explicit permutation against the plain-torch restatement (tests/edgepool_restatement.py),
   bit-equal, on both routes; each input's route is asserted.  The round count of a monotone path.
3. Route equality and run-to-run determinism, bitwise.
4. The scores against the float64 restatement at 1e-5, exactly 1 + add on targets with one incoming entry, the tie rule
   on a star and a tree.
5. The whole selector where no host order can be trusted: validity from the definition and equality with the
   restatement fed with the selector's own scores.
6. Degenerate inputs.
7. Gradients at fp32's own error, the one-launch Reduce + Connect of small-batch inference, callables, dropout.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import edgepool_restatement as R  # noqa: E402
from test_gpu_golden import check_output, check_so  # noqa: E402
from test_gpu_grad_paths import CAP, FACTOR, FLOOR, _graph_names, grad_path_errors  # noqa: E402
from test_gpu_kmis import hub_graph, make_batch  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = torch.load(os.path.join(HERE, "golden", "golden_edgepool_v1.pt"), weights_only=True)["cases"]
W, B = "selector.lin.weight", "selector.lin.bias"


def _dev():
    return torch.device("cuda:0")


def _method(name):
    from tgp.select import EdgeContractionSelect
    return getattr(EdgeContractionSelect, "compute_edge_score_" + name)


def _pool(c, dev, train=False):
    from tgp.poolers import EdgeContractionPooling
    pooler = EdgeContractionPooling(edge_score_method=_method(c["method"]), **c["cfg"]).to(dev)
    pooler = pooler.train() if train else pooler.eval()
    pooler.load_state_dict(c["params"])
    i = c["inputs"]
    kw = dict(adj=i["edge_index"].to(dev), edge_weight=None if i["edge_weight"] is None else i["edge_weight"].to(dev),
              batch=None if i["batch"] is None else i["batch"].to(dev))
    return pooler, kw


# ------------------------------------------------------------------------------------------------------ 1. fixtures
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_parity(name):
    c = CASES[name]
    dev = _dev()
    pooler, kw = _pool(c, dev)
    with torch.no_grad():
        out = pooler(x=c["inputs"]["x"].to(dev), **kw)
        score = pooler.selector.edge_scores(c["inputs"]["x"].to(dev), kw["adj"])
    e = dict(c["expected"])
    so = dict(e["so"])
    so["node_index"] = torch.arange(so["num_nodes"])
    torch.testing.assert_close(score.cpu(), e["score"], rtol=1e-5, atol=1e-5)
    check_so(out.so, so, name)
    check_output(out, e, name)
    want_route = "graphs" if c["inputs"]["batch"] is not None else "rounds"
    assert out.so.__dict__["_ec_route"] == want_route, name


# ------------------------------------------------------------------------------------------------------ inputs
def shuffled(ei, g):
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()


def run_both(ei, n, perm=None, score=None, ptr=None, gmax=None, expect="graphs"):
    """The matching on its natural route and forced device-wide; returns the two results (the second None when the
    natural route already is device-wide)."""
    from tgp import kernels
    first = kernels.edge_contract_select(ei, n, score, graph_ptr=ptr, max_graph_nodes=gmax, perm=perm)
    assert first.route == expect, (first.route, expect)
    second = None
    if expect == "graphs":
        second = kernels.edge_contract_select(ei, n, score, graph_ptr=ptr, max_graph_nodes=gmax, route="rounds", perm=perm)
        assert second.route == "rounds"
    return first, second


def assert_equals_restatement(res, ei, n, perm, what, score=None):
    """Device tensors: composed torch ops on integers, deterministic."""
    if perm is None and score is not None:
        perm = R.stable_perm(score)
    match = R.matching(ei, n, perm)
    cluster, k = R.clusters(ei, n, match)
    assert res.k == k, what
    assert torch.equal(res.matched.bool(), match), what
    assert torch.equal(res.match, match.nonzero().view(-1)), what
    assert torch.equal(res.index[1], cluster), what
    assert torch.equal(res.index[0], torch.arange(n, device=ei.device)), what
    if score is not None:
        assert torch.equal(res.weight, R.weights(ei, n, match, score)), what


SHAPES = {
    # name: (graphs, smallest, largest, out-degree, directed, shuffled, natural route)
    "small": (64, 20, 60, 2, False, False, "graphs"),  # random targets: duplicates and self-loops occur
    "medium": (8, 600, 1500, 2, False, False, "rounds"),  # past the per-graph limit of 1024 nodes
    "edge_cache": (1, 900, 900, 3, False, False, "graphs"),  # 5400 entries: beyond the 4096 kept in LDS
    "directed": (64, 20, 60, 3, True, False, "graphs"),
    "shuffled": (64, 20, 60, 2, False, True, "rounds"),  # not grouped by graph: declined, then device-wide
}


def shape_inputs(shape, seed, dev):
    graphs, lo, hi, deg, directed, shuf, route = SHAPES[shape]
    ei, batch, ptr, g = make_batch(graphs, lo, hi, deg, seed, directed=directed)
    if shuf:
        ei = shuffled(ei, g)
    gmax = int((ptr[1:] - ptr[:-1]).max())
    return ei.to(dev), batch.numel(), ptr.to(dev), gmax, route, g


# ------------------------------------------------------------------------------------------------------ 2. exactness
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_explicit_perm_both_routes(shape):
    from tgp import kernels
    dev = _dev()
    ei, n, ptr, gmax, route, g = shape_inputs(shape, 11, dev)
    if shape == "edge_cache":
        assert ei.size(1) > kernels.N.lib().tgp_edge_contract_edge_cache()
    if shape == "small":
        assert bool((ei[0] == ei[1]).any()), "the input was meant to hold self-loops"
    perm = torch.randperm(ei.size(1), generator=g).to(dev)
    for p in (perm, None):
        first, second = run_both(ei, n, perm=p, ptr=ptr, gmax=gmax, expect=route)
        assert_equals_restatement(first, ei, n, p, (shape, "natural"))
        if second is not None:
            assert_equals_restatement(second, ei, n, p, (shape, "rounds"))


def test_explicit_perm_hub_graph():
    """4 hubs of degree 3000 among 20 000 nodes, entries in random order: one lane per entry, no long rows."""
    from tgp.select import maximal_matching, maximal_matching_cluster
    dev = _dev()
    n = 20000
    ei, g = hub_graph(n, 120000, 4, 3000, 5)
    ei = ei.to(dev)
    assert int(torch.bincount(ei[1], minlength=n)[:4].min()) >= 3000
    perm = torch.randperm(ei.size(1), generator=g).to(dev)
    first, _ = run_both(ei, n, perm=perm, expect="rounds")
    assert_equals_restatement(first, ei, n, perm, "hub")
    match, cluster = maximal_matching_cluster(ei, n, perm)
    assert torch.equal(match, first.matched.bool()) and torch.equal(cluster, first.index[1])
    assert torch.equal(maximal_matching(ei, n, perm), match)


def test_monotone_path_takes_half_its_nodes_in_rounds():
    """130 nodes in a path whose scores fall along it: one entry per round is the minimum at both ends, so 65 rounds --
    a legitimate input, far inside the bound of num_nodes rounds."""
    dev = _dev()
    n = 130
    a = torch.arange(n - 1)
    ei = torch.stack([a, a + 1]).to(dev)
    score = torch.linspace(1.0, 0.0, n - 1).to(dev)
    ptr = torch.tensor([0, n], device=dev)
    first, second = run_both(ei, n, score=score, ptr=ptr, gmax=n, expect="graphs")
    for res in (first, second):
        assert res.rounds == 65 and res.k == 65, (res.route, res.rounds, res.k)
        assert_equals_restatement(res, ei, n, None, res.route, score=score)
    assert torch.equal(first.match, torch.arange(0, n - 1, 2, device=dev))


# ------------------------------------------------------------------------------------------------------ 3. routes
@pytest.mark.parametrize("shape", ["small", "edge_cache", "directed"])
def test_routes_agree_bitwise_and_runs_repeat(shape):
    """Scores quantised to 16 levels: every tie is decided by position, on both routes and on every run."""
    dev = _dev()
    ei, n, ptr, gmax, route, g = shape_inputs(shape, 23, dev)
    score = (torch.randint(0, 16, (ei.size(1),), generator=g).float() / 16).to(dev)
    runs = [run_both(ei, n, score=score, ptr=ptr, gmax=gmax, expect=route) for _ in range(2)]
    ref = runs[0][0]
    assert_equals_restatement(ref, ei, n, None, shape, score=score)
    for pair in runs:
        for res in pair:
            assert torch.equal(res.match, ref.match) and torch.equal(res.index, ref.index)
            assert torch.equal(res.weight, ref.weight) and res.k == ref.k


# ------------------------------------------------------------------------------------------------------ 4. scores
def degree_mix_graph(seed):
    """5000 nodes; target 0 has 3000 incoming entries (more than a workgroup takes in one pass of the hub kernel and far
    more than the 512 of the per-target pass), target 1 has 70 (more than a wave), targets 100..199 one each, the
    targets from 1000 on a random few.  Entries in random order."""
    g = torch.Generator().manual_seed(seed)
    n = 5000
    parts = [torch.stack([torch.randint(2, n, (3000,), generator=g), torch.zeros(3000, dtype=torch.long)]),
             torch.stack([torch.randint(2, n, (70,), generator=g), torch.ones(70, dtype=torch.long)]),
             torch.stack([torch.randint(0, n, (100,), generator=g), torch.arange(100, 200)]),
             torch.stack([torch.randint(0, n, (12000,), generator=g), torch.randint(1000, n, (12000,), generator=g)])]
    return shuffled(torch.cat(parts, 1), g), n, g


@pytest.mark.parametrize("F", [5, 48])
@pytest.mark.parametrize("method", R.METHODS)
def test_scores_against_float64(method, F):
    from tgp import kernels
    dev = _dev()
    ei, n, g = degree_mix_graph(3)
    indeg = torch.bincount(ei[1], minlength=n)
    assert int(indeg[0]) == 3000 and int(indeg[1]) == 70 and bool((indeg[100:200] == 1).all())
    x = torch.randn(n, F, generator=g)
    w = torch.randn(2 * F, generator=g) / F ** 0.5
    b = torch.randn(1, generator=g)
    add = 0.3
    got = kernels.edge_contract_scores(x.to(dev), ei.to(dev), w.to(dev), b.to(dev), method, add)
    want = R.scores(x.double(), ei, w.double(), b.double(), method, add)
    err = float((got.cpu().double() - want).abs().max())
    print(f"{method} F={F}: max |e - e64| = {err:.3e}")
    torch.testing.assert_close(got.cpu().double(), want, rtol=1e-5, atol=1e-5)
    raw = kernels.edge_contract_raw(x.to(dev), ei.to(dev), w.to(dev), b.to(dev))
    torch.testing.assert_close(raw.cpu().double(), R.raw_scores(x.double(), ei, w.double(), b.double()), rtol=1e-5,
                               atol=1e-5)
    again = kernels.edge_contract_scores(x.to(dev), ei.to(dev), w.to(dev), b.to(dev), method, add)
    assert torch.equal(got, again), "the scores are a pure function of the inputs"
    if method == "softmax":
        one = (indeg[ei[1]] == 1)
        assert int(one.sum()) >= 100
        exact = (torch.ones(1) + add).item()  # float32(1) + add, as torch adds a Python scalar to a float32 tensor
        assert bool((got.cpu()[one] == exact).all()), "a target with one incoming entry must score exactly 1 + add"


def star(leaves, g):
    hub = torch.zeros(leaves, dtype=torch.long)
    leaf = torch.arange(1, leaves + 1)
    return shuffled(torch.cat([torch.stack([hub, leaf]), torch.stack([leaf, hub])], 1), g), leaves + 1


def random_tree(n, g):
    child = torch.arange(1, n)
    parent = (torch.rand(n - 1, generator=g) * child).long()
    return shuffled(torch.cat([torch.stack([parent, child]), torch.stack([child, parent])], 1), g), n


@pytest.mark.parametrize("graph", ["star", "tree"])
def test_tie_rule_under_softmax(graph):
    """Every entry into a leaf is alone at its target and scores exactly 1.5, whatever the features: the order among
    them is the tie rule alone, lowest position first."""
    from tgp.select import EdgeContractionSelect
    dev = _dev()
    g = torch.Generator().manual_seed(17)
    ei, n = star(700, g) if graph == "star" else random_tree(900, g)
    x = torch.randn(n, 8, generator=g).to(dev)
    ei = ei.to(dev)
    sel = EdgeContractionSelect(8).to(dev).eval()
    with torch.no_grad():
        e = sel.edge_scores(x, ei)
        so = sel(x, ei)
    indeg = torch.bincount(ei[1], minlength=n)
    alone = indeg[ei[1]] == 1
    assert bool((e[alone] == 1.5).all()) and bool((e[~alone] < 1.5).all())
    res = so.__dict__["_ec_result"]
    assert_equals_restatement(res, ei, n, None, graph, score=e)
    if graph == "star":
        first = int(alone.nonzero()[0])  # the lowest hub -> leaf position
        assert res.match.tolist() == [first] and res.k == n - 1
        assert float(so.weight[0]) == 1.5 and float(so.weight[int(ei[1][first])]) == 1.5
        assert int((so.weight != 1).sum()) == 2


# ------------------------------------------------------------------------------------------------------ 5. selector
def assert_valid_maximal_matching(ei, n, matched):
    rows, cols = ei[0][matched], ei[1][matched]
    touched = torch.zeros(n, dtype=torch.long, device=ei.device)
    touched.index_add_(0, rows, torch.ones_like(rows))
    off = rows != cols
    touched.index_add_(0, cols[off], torch.ones_like(cols[off]))
    assert int(touched.max()) <= 1, "a node lies in two matched entries"
    assert bool((touched[ei[0]] + touched[ei[1]] > 0).all()), "an entry touches no matched node: not maximal"


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("shape", ["small", "medium", "directed"])
def test_whole_selector_is_valid_and_follows_its_own_order(shape, method):
    from tgp.select import EdgeContractionSelect
    dev = _dev()
    ei, n, ptr, gmax, route, g = shape_inputs(shape, 31, dev)
    batch = torch.repeat_interleave(torch.arange(ptr.numel() - 1, device=dev), ptr[1:] - ptr[:-1])
    x = torch.randn(n, 16, generator=g).to(dev)
    sel = EdgeContractionSelect(16, _method(method)).to(dev).eval()
    with torch.no_grad():
        e = sel.edge_scores(x, ei)
        so = sel(x, ei, batch=batch)
    res = so.__dict__["_ec_result"]
    assert res.route == route
    assert_valid_maximal_matching(ei, n, res.matched.bool())
    assert_equals_restatement(res, ei, n, None, (shape, method), score=e)
    assert torch.equal(so.cluster_index, res.index[1]) and torch.equal(so.weight, res.weight)
    assert so.num_supernodes == res.k == n - int((ei[0][res.match] != ei[1][res.match]).sum())


# ------------------------------------------------------------------------------------------------------ 6. degenerate
def test_degenerate_inputs():
    from tgp import kernels
    from tgp.poolers import EdgeContractionPooling
    from tgp.select import EdgeContractionSelect, maximal_matching, maximal_matching_cluster
    dev = _dev()
    sel = EdgeContractionSelect(4).to(dev).eval()
    none = torch.empty(2, 0, dtype=torch.long, device=dev)
    with torch.no_grad():
        # no edges: every node is a singleton with weight 1
        so = sel(torch.randn(7, 4, device=dev), none, batch=torch.tensor([0, 0, 0, 1, 1, 2, 2], device=dev))
        assert so.num_supernodes == 7 and torch.equal(so.cluster_index, torch.arange(7, device=dev))
        assert torch.equal(so.weight, torch.ones(7, device=dev))
        assert so.__dict__["_ec_result"].match.numel() == 0
        out = EdgeContractionPooling(4).to(dev).eval()(x=torch.randn(7, 4, device=dev), adj=none)
        assert out.x.shape == (7, 4) and out.edge_index.shape == (2, 0)
        # one node: alone, or matched with itself through a self-loop
        so = sel(torch.randn(1, 4, device=dev), none)
        assert so.num_supernodes == 1 and so.weight.tolist() == [1.0]
        loop = torch.zeros(2, 2, dtype=torch.long, device=dev)  # the self-loop twice: distinct ranks, one match
        so = sel(torch.randn(1, 4, device=dev), loop)
        res = so.__dict__["_ec_result"]
        assert so.num_supernodes == 1 and res.match.tolist() == [0]
        assert so.weight.tolist() == [1.0]  # softmax over the two entries: 0.5 + 0.5
        # isolated nodes stay singletons
        ei = torch.tensor([[1, 3, 3, 5], [3, 1, 5, 3]], device=dev)
        so = sel(torch.randn(8, 4, device=dev), ei)
        assert so.num_supernodes == 7 and bool((so.weight[[0, 2, 4, 6, 7]] == 1).all())
    assert maximal_matching(none, 3).shape == (0,)
    m, cl = maximal_matching_cluster(none, 3)
    assert m.shape == (0,) and torch.equal(cl, torch.arange(3, device=dev))
    res = kernels.edge_contract_select(none, 0, torch.empty(0, device=dev))
    assert res.k == 0 and res.index.shape == (2, 0)

    # an empty graph inside a sorted batch: the per-graph route skips it
    ei, batch, ptr, g = make_batch(6, 10, 30, 2, 41)
    sizes = ptr[1:] - ptr[:-1]
    ptr2 = torch.cat([ptr[:3], ptr[2:]])  # graph 2 is empty
    assert int((ptr2[1:] - ptr2[:-1]).min()) == 0
    ei, n = ei.to(dev), batch.numel()
    score = torch.rand(ei.size(1), generator=g).to(dev)
    first, second = run_both(ei, n, score=score, ptr=ptr2.to(dev), gmax=int(sizes.max()), expect="graphs")
    for res in (first, second):
        assert_equals_restatement(res, ei, n, None, "empty graph", score=score)

    # a list that is not grouped by graph is declined by the per-graph kernel and rerouted, not misread; asking for
    # the per-graph route explicitly raises
    bad = shuffled(ei.cpu(), g).to(dev)
    res = kernels.edge_contract_select(bad, n, score, graph_ptr=ptr.to(dev), max_graph_nodes=int(sizes.max()))
    assert res.route == "rounds"
    assert_equals_restatement(res, bad, n, None, "declined", score=score)
    with pytest.raises(kernels.N.TgpNativeError, match="declined"):
        kernels.edge_contract_select(bad, n, score, graph_ptr=ptr.to(dev), max_graph_nodes=int(sizes.max()), route="graphs")
    # an entry between two graphs: the same
    cross = ei.clone()
    cross[1, 0] = n - 1
    res = kernels.edge_contract_select(cross, n, score, graph_ptr=ptr.to(dev), max_graph_nodes=int(sizes.max()))
    assert res.route == "rounds"
    assert_equals_restatement(res, cross, n, None, "cross edge", score=score)
    # an unsorted batch vector never reaches the per-graph route
    with torch.no_grad():
        so = sel(torch.randn(n, 4, device=dev), ei, batch=batch.flip(0).to(dev))
    assert so.__dict__["_ec_route"] == "rounds"
    with pytest.raises(ValueError, match="one entry per edge"):
        kernels.edge_contract_select(ei, n, score[:-1])
    with pytest.raises(ValueError, match="route must be"):
        kernels.edge_contract_select(ei, n, score, route="fast")


# ------------------------------------------------------------------------------------------------------ 7. training
@pytest.mark.parametrize("name", sorted(CASES))
def test_gradients_against_the_float64_run(name):
    """d sum(x_pool^2) / d {x, lin.weight, lin.bias} against the fixture's float64 gradients, and the pooled features'
    path with the helper's random upstream gradient against the restatement: both at fp32's own error
    (max(FACTOR * e_oracle32, FLOOR), never above CAP).

    Under softmax the bias (and the target half of the weights) shifts every entry of a segment alike, so its gradient is
    zero in exact arithmetic and what float64 stores is rounding noise: there the bias is held to an absolute bound
    instead, max(FACTOR * |g32 - g64|, FLOOR * ||g64 of the weights||) -- the weight gradient is a sum of the same
    per-entry terms, so its norm is the scale the bias gradient's rounding lives on."""
    c = CASES[name]
    dev = _dev()
    i, cfg = c["inputs"], c["cfg"]
    softmax = c["method"] == "softmax"
    leaves = ["x", "w"] if softmax else ["x", "w", "b"]

    def kernel():
        pooler, kw = _pool(c, dev, train=True)
        x = i["x"].to(dev).requires_grad_(True)
        out = pooler(x=x, **kw)
        assert torch.equal(out.so.cluster_index.cpu(), c["expected"]["so"]["cluster_index"])
        names = _graph_names(out.x.grad_fn)
        assert "_EdgeScoreFnBackward" in names and "_EdgeWeightFnBackward" in names, names
        return {"x_pool": out.x}, {"x": x, "w": pooler.selector.lin.weight, "b": pooler.selector.lin.bias}

    def oracle(dtype):
        x = i["x"].to(dtype).requires_grad_(True)
        w = c["params"][W].to(dtype).requires_grad_(True)
        b = c["params"][B].to(dtype).requires_grad_(True)
        _, _, cluster, _, x_pool = R.pool(x, i["edge_index"], w, b, c["method"], cfg.get("add_to_edge_score", 0.5))
        assert torch.equal(cluster, c["expected"]["so"]["cluster_index"])
        return {"x_pool": x_pool}, {"x": x, "w": w, "b": b}

    report = []
    fails = grad_path_errors(name, kernel, oracle, leaves, report=report)
    for path, leaf, e_k, e_32 in report:
        print(f"{name} | {path} | {leaf} | e_kernel {e_k:.2e} | e_oracle32 {e_32:.2e}")
    assert not fails, "\n".join(fails)

    want = {"x": c["f64"]["grads"]["x"], "w": c["f64"]["grads"]["params"][W], "b": c["f64"]["grads"]["params"][B]}
    outs, lv = kernel()
    got = torch.autograd.grad((outs["x_pool"] ** 2).sum(), [lv["x"], lv["w"], lv["b"]])
    outs32, lv32 = oracle(torch.float32)
    g32 = torch.autograd.grad((outs32["x_pool"] ** 2).sum(), [lv32["x"], lv32["w"], lv32["b"]])
    for leaf, gk, go in zip(("x", "w", "b"), got, g32):
        ref = want[leaf].double()
        if leaf == "b" and softmax:
            scale = float(torch.linalg.vector_norm(want["w"].double()))
            a_k, a_32 = float((gk.cpu().double() - ref).abs().max()), float((go.double() - ref).abs().max())
            bound = max(FACTOR * a_32, FLOOR * scale)
            print(f"{name} | sum(x_pool^2) | b (zero in exact arithmetic) | |g - g64| {a_k:.2e} | oracle32 {a_32:.2e} | "
                  f"bound {bound:.2e}")
            assert a_k <= bound, (name, leaf, a_k, a_32, bound)
            continue
        e_k = float(torch.linalg.vector_norm(gk.cpu().double() - ref) / torch.linalg.vector_norm(ref))
        e_32 = float(torch.linalg.vector_norm(go.double() - ref) / torch.linalg.vector_norm(ref))
        bound = max(FACTOR * e_32, FLOOR)
        print(f"{name} | sum(x_pool^2) | {leaf} | e_kernel {e_k:.2e} | e_oracle32 {e_32:.2e} | bound {bound:.2e}")
        assert bound <= CAP and e_k <= bound, (name, leaf, e_k, e_32, bound)


def test_only_matched_entries_receive_a_gradient_from_the_weights():
    from tgp.select import EdgeContractionSelect
    dev = _dev()
    ei, n, ptr, gmax, route, g = shape_inputs("small", 51, dev)
    x = torch.randn(n, 8, generator=g).to(dev)
    sel = EdgeContractionSelect(8, _method("tanh")).to(dev).train()
    e = sel.edge_scores(x, ei)
    e.retain_grad()
    from tgp import kernels
    from tgp.select import _EdgeWeightFn
    res = kernels.edge_contract_select(ei, n, e.detach())
    up = torch.randn(n, generator=g).to(dev)
    (_EdgeWeightFn.apply(e, res.medge, res.weight) * up).sum().backward()
    want = torch.zeros_like(e)
    m = res.match
    loops = ei[0][m] == ei[1][m]
    want[m] = up[ei[0][m]] + torch.where(loops, torch.zeros_like(up[ei[1][m]]), up[ei[1][m]])
    torch.testing.assert_close(e.grad, want, rtol=1e-6, atol=1e-6)
    assert bool((e.grad[~res.matched.bool()] == 0).all())


def test_small_batch_inference_takes_the_one_launch_reduce_connect(monkeypatch):
    from tgp import kernels
    from tgp.poolers import EdgeContractionPooling
    dev = _dev()
    calls = []
    real = kernels.sparse_pool_small

    def counted(*a, **kw):
        out = real(*a, **kw)
        calls.append(out is not None)
        return out

    monkeypatch.setattr(kernels, "sparse_pool_small", counted)
    ei, batch, ptr, g = make_batch(256, 20, 60, 2, 95)
    n = batch.numel()
    x = torch.randn(n, 32, generator=g).to(dev)
    ew = (torch.rand(ei.size(1), generator=g) + 0.1).to(dev)
    ei, batch = ei.to(dev), batch.to(dev)
    pooler = EdgeContractionPooling(in_channels=32).to(dev).eval()
    with torch.no_grad():
        out = pooler(x=x, adj=ei, edge_weight=ew, batch=batch)
    assert calls == [True], "the one-launch Reduce + Connect was not taken"
    assert out.so.__dict__["_ec_route"] == "graphs"
    # the staged operators on the same selection: same pooled graph
    from tgp.connect import SparseConnect
    from tgp.reduce import BaseReduce
    with torch.no_grad():
        xp, bp = BaseReduce()(x, out.so, batch=batch)
        ei2, ew2 = SparseConnect()(ei, out.so, edge_weight=ew, batch_pooled=bp)
        lifted = pooler(x=out.x, so=out.so, lifting=True)
    assert torch.equal(out.edge_index, ei2) and torch.equal(out.batch, bp)
    torch.testing.assert_close(out.x, xp, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out.edge_weight, ew2, rtol=1e-5, atol=1e-5)
    # lifting=True: x_lifted = S x_pool, every node gets its cluster's row times its weight
    torch.testing.assert_close(lifted, out.x[out.so.cluster_index] * out.so.weight.view(-1, 1), rtol=1e-5, atol=1e-5)
    # training reaches the sparse Reduce's backward and the scorer trains
    pooler.train()
    out = pooler(x=x, adj=ei, edge_weight=ew, batch=batch)
    (out.x ** 2).sum().backward()
    gw = pooler.selector.lin.weight.grad
    assert gw is not None and torch.isfinite(gw).all() and gw.abs().sum() > 0


def test_user_callable_as_edge_score_method():
    from tgp.select import EdgeContractionSelect
    dev = _dev()
    seen = []

    def halved_tanh(raw, edge_index, num_nodes):
        seen.append((tuple(raw.shape), tuple(edge_index.shape), num_nodes))
        return torch.tanh(0.5 * raw)

    ei, n, ptr, gmax, route, g = shape_inputs("small", 61, dev)
    batch = torch.repeat_interleave(torch.arange(ptr.numel() - 1, device=dev), ptr[1:] - ptr[:-1])
    x = torch.randn(n, 12, generator=g).to(dev)
    sel = EdgeContractionSelect(12, halved_tanh, add_to_edge_score=0.25).to(dev).eval()
    with torch.no_grad():
        e = sel.edge_scores(x, ei)
        so = sel(x, ei, batch=batch)
    assert seen and seen[0] == ((ei.size(1),), (2, ei.size(1)), n)
    want = R.scores(x.cpu().double(), ei.cpu(), sel.lin.weight.detach().cpu().double(), sel.lin.bias.detach().cpu().double(),
                    halved_tanh, 0.25)
    torch.testing.assert_close(e.cpu().double(), want, rtol=1e-5, atol=1e-5)
    res = so.__dict__["_ec_result"]
    assert res.route == "graphs"
    assert_equals_restatement(res, ei, n, None, "callable", score=e)
    # and it trains: the callable is a torch function of the natively computed raw scores
    sel.train()
    so = sel(x, ei, batch=batch)
    so.weight.sum().backward()
    assert sel.lin.weight.grad is not None and sel.lin.weight.grad.abs().sum() > 0


def test_static_score_methods_are_callable_on_their_own():
    """The three ``compute_edge_score_*`` methods as the reference exposes them: plain functions of the raw scores (tanh
    and sigmoid without a graph), differentiable, usable inside a user callable."""
    from tgp.select import EdgeContractionSelect as S
    dev = _dev()
    ei, n, ptr, gmax, route, g = shape_inputs("directed", 81, dev)
    raw = torch.randn(ei.size(1), generator=g).to(dev).requires_grad_(True)
    raw64 = raw.detach().cpu().double().requires_grad_(True)
    up = torch.randn(ei.size(1), generator=g)
    for name, got in (("softmax", S.compute_edge_score_softmax(raw, ei, n)), ("tanh", S.compute_edge_score_tanh(raw)),
                      ("sigmoid", S.compute_edge_score_sigmoid(raw))):
        want = R.normalize(raw64, ei.cpu(), n, name, 0.0)
        torch.testing.assert_close(got.detach().cpu().double(), want.detach(), rtol=1e-5, atol=1e-5)
        gk, = torch.autograd.grad(got, raw, up.to(dev))
        g64, = torch.autograd.grad(want, raw64, up.double())
        torch.testing.assert_close(gk.cpu().double(), g64, rtol=1e-4, atol=1e-5)
    sel = S(8, lambda r, e, k: 2.0 * S.compute_edge_score_softmax(r, e, k)).to(dev).eval()
    x = torch.randn(n, 8, generator=g).to(dev)
    with torch.no_grad():
        doubled = sel.edge_scores(x, ei)
        plain = S(8).to(dev).eval()
        plain.load_state_dict(sel.state_dict())
        torch.testing.assert_close(doubled, 2.0 * (plain.edge_scores(x, ei) - 0.5) + 0.5, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("method", ["softmax", "sigmoid"])
def test_dropout_in_training_uses_torch_dropout_between_the_two_native_stages(method):
    from tgp import kernels
    from tgp.select import EdgeContractionSelect
    dev = _dev()
    ei, n, ptr, gmax, route, g = shape_inputs("small", 71, dev)
    x = torch.randn(n, 8, generator=g).to(dev)
    sel = EdgeContractionSelect(8, _method(method), dropout=0.3).to(dev).train()
    torch.manual_seed(1234)
    e = sel.edge_scores(x, ei)
    torch.manual_seed(1234)
    so = sel(x, ei)
    with torch.no_grad():
        raw = kernels.edge_contract_raw(x, ei, sel.lin.weight, sel.lin.bias)
        torch.manual_seed(1234)
        dropped = torch.nn.functional.dropout(raw, p=0.3, training=True)
        assert 0.15 < float((dropped == 0).float().mean()) < 0.45
        want = R.normalize(dropped.cpu().double(), ei.cpu(), n, method, 0.5)
    torch.testing.assert_close(e.detach().cpu().double(), want, rtol=1e-5, atol=1e-5)
    res = so.__dict__["_ec_result"]
    assert_equals_restatement(res, ei, n, None, "dropout", score=e.detach())
    so.weight.sum().backward()
    assert sel.lin.weight.grad is not None and torch.isfinite(sel.lin.weight.grad).all()
    # in eval mode nothing is dropped
    sel.eval()
    with torch.no_grad():
        e_eval = sel.edge_scores(x, ei)
        torch.testing.assert_close(e_eval, kernels.edge_contract_scores(x, ei, sel.lin.weight, sel.lin.bias, method, 0.5),
                                   rtol=0, atol=0)
