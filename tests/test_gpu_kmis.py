"""k-MIS pooling on the GPU (csrc/kmis_select.hip through tgp.kernels / KMISSelect / KMISPooling).

1. Fixture parity with the reference (tests/golden/golden_kmis_v1.pt): indices exact, values at rtol = atol = 1e-5.
2. Exactness with an explicit permutation against the plain-torch restatement (tests/kmis_restatement.py), bit-equal, on
   both routes; each input's route is asserted.
3. The heuristics alone: "greedy" bit-equal (integer counts, one correctly rounded division), "w-greedy" and the "degree"
   scorer at 1e-5.
4. Route equality and run-to-run determinism, bitwise.
5. The whole selector where no host order can be trusted: validity by dense reachability matrices (written apart from the
   restatement) and equality with the explicit-permutation entry fed with the stable order of the selector's own scores.
6. Degenerate inputs.
7. Gradients against the fixtures' float64 run, and the one-launch Reduce + Connect of small-batch inference.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kmis_restatement as R  # noqa: E402
from test_gpu_golden import check_output, check_so  # noqa: E402
from test_gpu_grad_paths import CAP, FACTOR, FLOOR, _graph_names, grad_path_errors  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = torch.load(os.path.join(HERE, "golden", "golden_kmis_v1.pt"), weights_only=True)["cases"]
LINEAR = sorted(n for n in CASES if CASES[n]["cfg"].get("scorer", "linear") == "linear")


def _dev():
    return torch.device("cuda:0")


def _pool(c, dev, train=False):
    from tgp.poolers import KMISPooling
    pooler = KMISPooling(**c["cfg"]).to(dev)
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
    e = dict(c["expected"])
    so = dict(e["so"])
    so["node_index"] = torch.arange(so["num_nodes"])
    if c["cfg"].get("scorer") == "canonical":  # the one stated difference: the reference's scores are int64 there
        assert so["weight"].dtype == torch.int64 and out.so.weight.dtype == torch.float32
        so["weight"] = so["weight"].to(torch.float32)
    check_so(out.so, so, name)
    assert torch.equal(out.so.mis.cpu(), so["mis"]), name
    check_output(out, e, name)
    torch.testing.assert_close(out.x.cpu(), e["x"], rtol=1e-5, atol=1e-5)
    if e["batch"] is None:
        assert out.batch is None
    else:
        assert torch.equal(out.batch.cpu(), e["batch"])


# ------------------------------------------------------------------------------------------------------ inputs
def make_batch(num_graphs, lo, hi, deg, seed, directed=False):
    """A sorted batch on the host: (edge_index grouped by source node, batch, ptr).  Random targets inside each graph:
    duplicates and self-loops occur."""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(lo, hi + 1, (num_graphs,), generator=g)
    ptr = torch.zeros(num_graphs + 1, dtype=torch.long)
    ptr[1:] = sizes.cumsum(0)
    n = int(ptr[-1])
    batch = torch.repeat_interleave(torch.arange(num_graphs), sizes)
    src = torch.arange(n).repeat_interleave(deg)
    dst = ptr[batch[src]] + (torch.rand(src.numel(), generator=g) * sizes[batch[src]]).long().clamp(max=hi - 1)
    dst = torch.minimum(dst, ptr[batch[src] + 1] - 1)
    ei = torch.stack([src, dst])
    if not directed:
        ei = torch.cat([ei, ei.flip(0)], 1)
    order = torch.sort(ei[0], stable=True)[1]
    return ei[:, order].contiguous(), batch, ptr, g


def hub_graph(n, e, hubs, hub_deg, seed):
    g = torch.Generator().manual_seed(seed)
    m = e // 2 - hubs * hub_deg
    a = torch.randint(0, n, (2, m), generator=g)
    h = torch.stack([torch.arange(hubs).repeat_interleave(hub_deg), torch.randint(hubs, n, (hubs * hub_deg,), generator=g)])
    ei = torch.cat([a, h], 1)
    ei = torch.cat([ei, ei.flip(0)], 1)
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous(), g


def path_graph(n, offset=0):
    a = torch.arange(n - 1) + offset
    return torch.cat([torch.stack([a, a + 1]), torch.stack([a + 1, a])], 1)


def run_both(ei, n, k, perm=None, score=None, heuristic=None, ptr=None, gmax=None, expect="graphs"):
    """The selection on its natural route and forced device-wide; returns the two results (the second None when the
    natural route already is device-wide)."""
    from tgp import kernels
    first = kernels.kmis_select(ei, n, k, score=score, heuristic=heuristic, perm=perm, graph_ptr=ptr, max_graph_nodes=gmax)
    assert first.route == expect, (first.route, expect)
    second = None
    if expect == "graphs":
        second = kernels.kmis_select(ei, n, k, score=score, heuristic=heuristic, perm=perm, graph_ptr=ptr,
                                     max_graph_nodes=gmax, route="rounds")
        assert second.route == "rounds"
    return first, second


def assert_equals_restatement(res, ei, n, k, perm, what):
    mis, cluster = R.mis_cluster(ei, k, perm, n)  # (device tensors: composed torch ops on integers, deterministic)
    assert res.k == int(mis.sum()), what
    assert torch.equal(res.mis, mis.nonzero().view(-1)), what
    assert torch.equal(res.index[1], cluster), what
    assert torch.equal(res.index[0], torch.arange(n, device=ei.device)), what


# ------------------------------------------------------------------------------------------------------ 2. exactness
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("shape", ["small", "medium"])
def test_explicit_perm_batches_both_routes(shape, k):
    dev = _dev()
    ei, batch, ptr, g = make_batch(2048, 20, 60, 2, 11 + k) if shape == "small" else make_batch(64, 600, 1000, 3, 21 + k)
    n = batch.numel()
    perm = torch.randperm(n, generator=g).to(dev)
    ei, ptr = ei.to(dev), ptr.to(dev)
    gmax = 60 if shape == "small" else 1000
    a, b = run_both(ei, n, k, perm=perm, ptr=ptr, gmax=gmax, expect="graphs")
    assert_equals_restatement(a, ei, n, k, perm, f"{shape} k={k} graphs")
    assert_equals_restatement(b, ei, n, k, perm, f"{shape} k={k} rounds")


@pytest.mark.parametrize("k", [1, 2, 3])
def test_explicit_perm_hub_graph(k):
    from tgp.select import maximal_independent_set_cluster
    dev = _dev()
    n = 200_000
    ei, g = hub_graph(n, 2_000_000, 10, 20_000, 31)
    assert ei.size(1) == 2_000_000 and int(torch.bincount(ei[1], minlength=n)[:10].min()) >= 20_000
    perm = torch.randperm(n, generator=g).to(dev)
    ei = ei.to(dev)
    a, _ = run_both(ei, n, k, perm=perm, expect="rounds")
    assert_equals_restatement(a, ei, n, k, perm, f"hubs k={k}")
    if k == 1:
        mis, cluster = maximal_independent_set_cluster(ei, k, perm, n)
        assert torch.equal(mis.nonzero().view(-1), a.mis) and torch.equal(cluster, a.index[1])


@pytest.mark.parametrize("k", [1, 2, 3])
def test_explicit_perm_directed(k):
    from tgp.select import maximal_independent_set
    dev = _dev()
    ei, batch, ptr, g = make_batch(300, 10, 200, 2, 41, directed=True)
    n = batch.numel()
    perm = torch.randperm(n, generator=g).to(dev)
    ei, ptr = ei.to(dev), ptr.to(dev)
    a, b = run_both(ei, n, k, perm=perm, ptr=ptr, gmax=200, expect="graphs")
    assert_equals_restatement(a, ei, n, k, perm, f"directed k={k} graphs")
    assert_equals_restatement(b, ei, n, k, perm, f"directed k={k} rounds")
    mis = maximal_independent_set(ei, k, perm, n)  # (no batch: device-wide)
    assert torch.equal(mis.nonzero().view(-1), a.mis)


def test_paths_take_one_node_per_round():
    """perm = arange, order_k = 1 on a path: one new member per round, n / 2 rounds -- the worst case of both loops."""
    dev = _dev()
    n1 = 1000
    ei = torch.cat([path_graph(n1), path_graph(6, n1)], 1).to(dev)  # a second small graph: a batch, per-graph route
    ptr = torch.tensor([0, n1, n1 + 6], device=dev)
    a, b = run_both(ei, n1 + 6, 1, perm=torch.arange(n1 + 6, device=dev), ptr=ptr, gmax=n1, expect="graphs")
    want = torch.cat([torch.arange(0, n1, 2), torch.arange(n1, n1 + 6, 2)]).to(dev)
    for res in (a, b):
        assert torch.equal(res.mis, want)
        assert torch.equal(res.index[1], torch.arange(n1 + 6, device=dev) // 2)
    assert b.rounds >= n1 // 2
    n2 = 5000
    ei = path_graph(n2).to(dev)
    c, _ = run_both(ei, n2, 1, perm=None, expect="rounds")
    assert torch.equal(c.mis, torch.arange(0, n2, 2, device=dev))
    assert torch.equal(c.index[1], torch.arange(n2, device=dev) // 2)
    assert c.rounds >= n2 // 2
    assert_equals_restatement(a, torch.cat([path_graph(n1), path_graph(6, n1)], 1).to(dev), n1 + 6, 1, None, "path")


# ------------------------------------------------------------------------------------------------------ 3. heuristics
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_heuristics_and_degree_scorer(k, directed):
    from tgp import kernels
    from tgp.select import degree_scorer
    dev = _dev()
    ei, batch, ptr, g = make_batch(200, 5, 80, 2, 51 + k, directed=directed)  # duplicates and self-loops among them
    n = batch.numel()
    score = torch.rand(n, generator=g) + 0.05
    ew = torch.rand(ei.size(1), generator=g) + 0.1
    got = kernels.kmis_updated_score(score.to(dev), ei.to(dev), k, "greedy").cpu()
    want = R.updated_score(score, ei, k, "greedy")
    assert float(R.k_sums(score, ei, k, "greedy").max()) < 2 ** 24
    assert torch.equal(got, want), "greedy: integer counts and one division leave no room"
    res = kernels.kmis_select(ei.to(dev), n, k, score=score.to(dev), heuristic="greedy", graph_ptr=ptr.to(dev),
                              max_graph_nodes=80)
    assert res.route == "graphs" and torch.equal(res.updated.cpu(), want)
    got = kernels.kmis_updated_score(score.to(dev), ei.to(dev), k, "w-greedy").cpu()
    torch.testing.assert_close(got, R.updated_score(score, ei, k, "w-greedy"), rtol=1e-5, atol=1e-5)
    for w in (ew, None):
        deg = degree_scorer(ei.to(dev), None if w is None else w.to(dev), n).cpu()
        ref = torch.zeros(n).index_add(0, ei[1], torch.ones(ei.size(1)) if w is None else w)
        torch.testing.assert_close(deg, ref, rtol=1e-5, atol=1e-5)
    out_deg = degree_scorer(ei.to(dev), ew.to(dev), n, dim=0).cpu()
    torch.testing.assert_close(out_deg, torch.zeros(n).index_add(0, ei[0], ew), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------------ 4. routes
@pytest.mark.parametrize("heuristic", [None, "greedy", "w-greedy"])
@pytest.mark.parametrize("shape", ["small", "medium"])
def test_routes_agree_bitwise_and_runs_repeat(shape, heuristic):
    dev = _dev()
    ei, batch, ptr, g = make_batch(2048, 20, 60, 2, 61) if shape == "small" else make_batch(64, 600, 1000, 3, 62)
    n = batch.numel()
    score = (torch.rand(n, generator=g) + 0.05).to(dev)
    if heuristic is None:
        score = (score * 8).round() / 8  # many exact ties: the tie rule is part of what must agree
    ei, ptr = ei.to(dev), ptr.to(dev)
    gmax = 60 if shape == "small" else 1000
    for k in (1, 2):
        a, b = run_both(ei, n, k, score=score, heuristic=heuristic, ptr=ptr, gmax=gmax, expect="graphs")
        a2, b2 = run_both(ei, n, k, score=score, heuristic=heuristic, ptr=ptr, gmax=gmax, expect="graphs")
        for other in (b, a2, b2):
            assert other.k == a.k
            assert torch.equal(other.mis, a.mis) and torch.equal(other.index, a.index)
            assert torch.equal(other.updated.view(torch.int32), a.updated.view(torch.int32))
        perm = R.stable_perm(a.updated)
        assert_equals_restatement(a, ei, n, k, perm, f"{shape} {heuristic} k={k}")


# ------------------------------------------------------------------------------------------------------ 5. selector
def dense_reach(ei, batch, ptr, k):
    """[B, M, M] bool on the host: reach[g, i, j] = local node i reaches local node j within k hops (row -> col)."""
    b = ptr.numel() - 1
    m = int((ptr[1:] - ptr[:-1]).max())
    adj = torch.zeros(b, m, m)
    gi = batch[ei[0]]
    adj[gi, ei[0] - ptr[gi], ei[1] - ptr[gi]] = 1.0
    adj = ((adj + torch.eye(m)) > 0).float()
    reach = torch.eye(m).expand(b, m, m).clone()
    for _ in range(k):
        reach = (torch.bmm(reach, adj) > 0).float()
    return reach > 0


def assert_valid_selection(mis_idx, cluster, ei, batch, ptr, k, undirected):
    n = batch.numel()
    reach = dense_reach(ei, batch, ptr, k)
    mis = torch.zeros(n, dtype=torch.bool)
    mis[mis_idx] = True
    assert torch.equal(mis_idx, mis.nonzero().view(-1)), "members not in ascending node order"
    assert torch.equal(cluster[mis_idx], torch.arange(mis_idx.numel())), "ids do not number the members in ascending order"
    local = torch.arange(n) - ptr[batch]
    m = reach.size(1)
    member = torch.zeros(reach.size(0), m, dtype=torch.bool)
    member[batch[mis_idx], local[mis_idx]] = True
    from_members = reach & member.unsqueeze(2)  # rows of members only
    covered = from_members.any(1)
    assert bool(covered[batch, local].all()), "not maximal: a node no member reaches"
    between = from_members & member.unsqueeze(1)
    between = between & ~torch.eye(m, dtype=torch.bool)
    if undirected:
        assert not bool(between.any()), "not independent: two members within k hops"
    else:
        assert not bool((between & between.transpose(1, 2)).any())
    owner = mis_idx[cluster]
    assert torch.equal(batch[owner], batch), "a node assigned across graphs"
    assert bool(reach[batch, local[owner], local].all()), "a node whose member does not reach it within k hops"


@pytest.mark.parametrize("scorer,heuristic,k", [("random", "greedy", 1), ("constant", "greedy", 2), ("degree", None, 1),
                                                ("degree", "w-greedy", 2), ("linear", "greedy", 2),
                                                ("linear", "w-greedy", 1), ("constant", None, 3)])
def test_whole_selector_is_valid_and_follows_its_own_order(scorer, heuristic, k):
    from tgp import kernels
    from tgp.select import KMISSelect
    dev = _dev()
    ei, batch, ptr, g = make_batch(2048, 20, 60, 2, 71)
    n = batch.numel()
    assert 70_000 < n < 90_000
    x = torch.randn(n, 16, generator=g)
    ew = torch.rand(ei.size(1), generator=g) + 0.1
    sel = KMISSelect(in_channels=16, order_k=k, scorer=scorer, score_heuristic=heuristic).to(dev)
    for with_batch in (True, False):
        with torch.no_grad():
            so = sel(edge_index=ei.to(dev), edge_weight=ew.to(dev), x=x.to(dev),
                     batch=batch.to(dev) if with_batch else None, num_nodes=n)
        assert so.__dict__["_kmis_route"] == ("graphs" if with_batch else "rounds")
        assert so.num_supernodes == so.mis.numel() and so.weight.shape == (n,)
        assert_valid_selection(so.mis.cpu(), so.cluster_index.cpu(), ei, batch, ptr, k, undirected=True)
        upd = so.__dict__["_kmis_updated"]
        res = kernels.kmis_select(ei.to(dev), n, k, perm=R.stable_perm(upd))
        assert torch.equal(res.mis, so.mis) and torch.equal(res.index[1], so.cluster_index)


# ------------------------------------------------------------------------------------------------------ 6. degenerate
def test_degenerate_inputs():
    from tgp import kernels
    from tgp.select import KMISSelect, maximal_independent_set, maximal_independent_set_cluster
    dev = _dev()
    empty = torch.empty(2, 0, dtype=torch.long, device=dev)
    # E = 0: every node is its own supernode, with and without a batch
    mis, cluster = maximal_independent_set_cluster(empty, 2, None, 7)
    assert mis.all() and cluster.tolist() == list(range(7))
    res = kernels.kmis_select(empty, 7, 1, graph_ptr=torch.tensor([0, 3, 7], device=dev), max_graph_nodes=4)
    assert res.route == "graphs" and res.k == 7 and res.index[1].tolist() == list(range(7))
    # N = 0
    mis, cluster = maximal_independent_set_cluster(empty, 1, None, 0)
    assert mis.numel() == 0 and cluster.numel() == 0 and mis.dtype == torch.bool
    so = KMISSelect(scorer="constant")(edge_index=empty, num_nodes=0)
    assert so.num_nodes == 0 and so.num_supernodes == 0
    # isolated nodes, self-loops and duplicates, an unsorted edge list
    g = torch.Generator().manual_seed(5)
    ei = torch.tensor([[0, 1, 1, 2, 2, 2, 4, 4, 5, 7, 7, 8], [1, 0, 1, 2, 4, 4, 2, 2, 5, 8, 8, 7]])
    ei = ei[:, torch.randperm(ei.size(1), generator=g)].to(dev)  # nodes 3, 6 isolated; 5 has only a self-loop
    for k in (1, 2):
        perm = torch.randperm(10, generator=g).to(dev)
        res = kernels.kmis_select(ei, 10, k, perm=perm)
        assert res.route == "rounds"
        assert_equals_restatement(res, ei, 10, k, perm, "unsorted list")
        for lone in (3, 5, 6, 9):
            assert lone in res.mis.tolist()
    # the same unsorted list as a one-graph batch: the per-graph kernel takes it (its edges all lie in its graph)
    res = kernels.kmis_select(ei, 10, 1, graph_ptr=torch.tensor([0, 10], device=dev), max_graph_nodes=10)
    assert res.route == "graphs"
    assert_equals_restatement(res, ei, 10, 1, None, "one-graph batch")
    # an unsorted batch vector: device-wide through the selector
    batch = torch.tensor([1, 1, 1, 0, 1, 0, 0, 2, 2, 2], device=dev)
    so = KMISSelect(scorer="canonical", score_heuristic=None)(edge_index=ei, batch=batch, num_nodes=10)
    assert so.__dict__["_kmis_route"] == "rounds"
    mis, cluster = R.mis_cluster(ei, 1, None, 10)
    assert torch.equal(so.mis, mis.nonzero().view(-1)) and torch.equal(so.cluster_index, cluster)
    assert so.weight.dtype == torch.float32 and so.weight.tolist() == [-float(i) for i in range(10)]
    # an edge between two graphs of a sorted batch: the per-graph kernel declines, the result is still exact
    ei2, b2, ptr2, g2 = make_batch(50, 10, 40, 2, 81)
    n2 = b2.numel()
    cross = torch.tensor([[int(ptr2[3])], [int(ptr2[7])]])
    where = int((ei2[0] <= cross[0, 0]).sum())
    ei2 = torch.cat([ei2[:, :where], cross, ei2[:, where:]], 1).to(dev)  # still grouped by source node
    perm = torch.randperm(n2, generator=g2).to(dev)
    res = kernels.kmis_select(ei2, n2, 2, perm=perm, graph_ptr=ptr2.to(dev), max_graph_nodes=40)
    assert kernels.kmis_route(n2, ei2.size(1), ptr2.to(dev), 40) == "graphs" and res.route == "rounds"
    assert_equals_restatement(res, ei2, n2, 2, perm, "cross-graph edge")
    with pytest.raises(Exception, match="declined"):
        kernels.kmis_select(ei2, n2, 2, perm=perm, graph_ptr=ptr2.to(dev), max_graph_nodes=40, route="graphs")
    # order_k beyond every diameter: one supernode per connected component
    ei3 = torch.cat([path_graph(30), path_graph(12, 30), path_graph(5, 42)], 1).to(dev)
    for ptr3 in (None, torch.tensor([0, 30, 42, 50], device=dev)):
        res = kernels.kmis_select(ei3, 50, 64, graph_ptr=ptr3, max_graph_nodes=None if ptr3 is None else 30)
        assert res.mis.tolist() == [0, 30, 42, 47, 48, 49]
        assert res.index[1].tolist() == [0] * 30 + [1] * 12 + [2] * 5 + [3, 4, 5]
    assert maximal_independent_set(ei3, 64, None, 50).nonzero().view(-1).tolist() == [0, 30, 42, 47, 48, 49]


def test_force_undirected_and_coo_input():
    from tgp.select import KMISSelect
    dev = _dev()
    ei, batch, ptr, g = make_batch(20, 10, 30, 2, 91, directed=True)
    n = batch.numel()
    keep = ei[0] != ei[1]
    ei = torch.unique(ei[:, keep], dim=1)
    ew = torch.rand(ei.size(1), generator=g) + 0.1
    both = torch.unique(torch.cat([ei, ei.flip(0)], 1), dim=1)
    sel = KMISSelect(order_k=2, scorer="constant", force_undirected=True)
    so = sel(edge_index=ei.to(dev), edge_weight=ew.to(dev), batch=batch.to(dev), num_nodes=n)
    mis, cluster, _ = R.select(torch.ones(n), both, 2, "greedy", n)
    assert torch.equal(so.mis.cpu(), mis) and torch.equal(so.cluster_index.cpu(), cluster)
    coo = torch.sparse_coo_tensor(both, torch.ones(both.size(1)), (n, n)).coalesce().to(dev)
    so2 = KMISSelect(order_k=2, scorer="constant")(edge_index=coo, batch=batch.to(dev))
    assert torch.equal(so2.mis, so.mis) and torch.equal(so2.cluster_index, so.cluster_index)


# ------------------------------------------------------------------------------------------------------ 7. training
@pytest.mark.parametrize("name", LINEAR)
def test_gradients_against_the_float64_run(name):
    """d sum(x_pool^2) / d {x, lin.weight, lin.bias} against the fixture's float64 gradients, and the pooled features'
    path with the helper's random upstream gradient against the restatement: both at fp32's own error
    (max(FACTOR * e_oracle32, FLOOR), never above CAP)."""
    c = CASES[name]
    dev = _dev()
    i, cfg = c["inputs"], c["cfg"]
    k, h = cfg.get("order_k", 1), cfg.get("score_heuristic", "greedy")
    none = cfg.get("reduce_red_op", "sum") is None
    wname, bname = "selector.lin.weight", "selector.lin.bias"

    def kernel():
        pooler, kw = _pool(c, dev, train=True)
        x = i["x"].to(dev).requires_grad_(True)
        out = pooler(x=x, **kw)
        assert torch.equal(out.so.mis.cpu(), c["expected"]["so"]["mis"])
        if not none:
            assert "_SparseReduceFnBackward" in _graph_names(out.x.grad_fn)
        return {"x_pool": out.x}, {"x": x, "w": pooler.selector.lin.weight, "b": pooler.selector.lin.bias}

    def oracle(dtype):
        x = i["x"].to(dtype).requires_grad_(True)
        w = c["params"][wname].to(dtype).requires_grad_(True)
        b = c["params"][bname].to(dtype).requires_grad_(True)
        ew = i["edge_weight"]
        _, mis, _, x_pool = R.pool(x, i["edge_index"], None if ew is None else ew.to(dtype), i["batch"], w, b, k, h,
                                   reduce_none=none)
        assert torch.equal(mis, c["expected"]["so"]["mis"])
        return {"x_pool": x_pool}, {"x": x, "w": w, "b": b}

    report = []
    fails = grad_path_errors(name, kernel, oracle, ["x", "w", "b"], report=report)
    for path, leaf, e_k, e_32 in report:
        print(f"{name} | {path} | {leaf} | e_kernel {e_k:.2e} | e_oracle32 {e_32:.2e}")
    assert not fails, "\n".join(fails)

    want = {"x": c["f64"]["grads"]["x"], "w": c["f64"]["grads"]["params"][wname], "b": c["f64"]["grads"]["params"][bname]}
    outs, lv = kernel()
    got = torch.autograd.grad((outs["x_pool"] ** 2).sum(), [lv["x"], lv["w"], lv["b"]])
    outs32, lv32 = oracle(torch.float32)
    g32 = torch.autograd.grad((outs32["x_pool"] ** 2).sum(), [lv32["x"], lv32["w"], lv32["b"]])
    for leaf, gk, go in zip(("x", "w", "b"), got, g32):
        ref = want[leaf].double()
        e_k = float(torch.linalg.vector_norm(gk.cpu().double() - ref) / torch.linalg.vector_norm(ref))
        e_32 = float(torch.linalg.vector_norm(go.double() - ref) / torch.linalg.vector_norm(ref))
        bound = max(FACTOR * e_32, FLOOR)
        print(f"{name} | sum(x_pool^2) | {leaf} | e_kernel {e_k:.2e} | e_oracle32 {e_32:.2e} | bound {bound:.2e}")
        assert bound <= CAP and e_k <= bound, (name, leaf, e_k, e_32, bound)


def test_small_batch_inference_takes_the_one_launch_reduce_connect(monkeypatch):
    from tgp import kernels
    from tgp.poolers import KMISPooling
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
    pooler = KMISPooling(in_channels=32, order_k=2).to(dev).eval()
    with torch.no_grad():
        out = pooler(x=x, adj=ei, edge_weight=ew, batch=batch)
    assert calls == [True], "the one-launch Reduce + Connect was not taken"
    assert out.so.__dict__["_kmis_route"] == "graphs"
    # the staged operators on the same selection: same pooled graph
    from tgp.connect import SparseConnect
    from tgp.reduce import BaseReduce
    with torch.no_grad():
        xp, bp = BaseReduce()(x, out.so, batch=batch)
        ei2, ew2 = SparseConnect()(ei, out.so, edge_weight=ew, batch_pooled=bp)
    assert torch.equal(out.edge_index, ei2) and torch.equal(out.batch, bp)
    torch.testing.assert_close(out.x, xp, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out.edge_weight, ew2, rtol=1e-5, atol=1e-5)
    # training reaches the sparse Reduce's backward and the scorer trains
    pooler.train()
    out = pooler(x=x, adj=ei, edge_weight=ew, batch=batch)
    (out.x ** 2).sum().backward()
    gw = pooler.selector.lin.weight.grad
    assert gw is not None and torch.isfinite(gw).all() and gw.abs().sum() > 0
