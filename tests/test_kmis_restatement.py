"""The plain-torch restatement of k-MIS selection (tests/kmis_restatement.py, ties to the lower node index) against the
reference's stored results (tests/golden/golden_kmis_v1.pt: cases whose order is tie-free or, up to 16 nodes, stable in the
reference too), against a sequential greedy walk, and against the definition (independent, maximal, clusters reached
within k hops) on boolean reachability matrices.  The GPU tests then hold the kernels to this restatement bit for bit."""
import os

import pytest
import torch

import kmis_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_kmis_v1.pt"), weights_only=True)["cases"]


def scores_of(c, dtype):
    """The case's scores in ``dtype`` (linear scorer: from the stored parameters; else the stored weights)."""
    i, cfg = c["inputs"], c["cfg"]
    if cfg.get("scorer", "linear") == "linear":
        w, b = c["params"]["selector.lin.weight"].to(dtype), c["params"]["selector.lin.bias"].to(dtype)
        return torch.sigmoid(i["x"].to(dtype) @ w.t() + b).view(-1)
    return c["expected"]["so"]["weight"].to(dtype)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference(name):
    c = CASES[name]
    i, cfg, e = c["inputs"], c["cfg"], c["expected"]
    n = i["x"].size(0)
    k, h = cfg.get("order_k", 1), cfg.get("score_heuristic", "greedy")
    score = scores_of(c, torch.float32)
    torch.testing.assert_close(score, e["so"]["weight"].to(torch.float32), rtol=1e-6, atol=1e-6)
    mis, cluster, _ = R.select(score, i["edge_index"], k, h, n)
    assert torch.equal(mis, e["so"]["mis"]), name
    assert torch.equal(cluster, e["so"]["cluster_index"]), name
    assert e["so"]["num_supernodes"] == mis.numel()


@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n]["cfg"].get("scorer", "linear") == "linear"))
def test_restatement_matches_the_float64_run(name):
    c = CASES[name]
    i, cfg, f = c["inputs"], c["cfg"], c["f64"]
    ew = i["edge_weight"]
    score, mis, cluster, x_pool = R.pool(
        i["x"].double(), i["edge_index"], None if ew is None else ew.double(), i["batch"],
        c["params"]["selector.lin.weight"].double(), c["params"]["selector.lin.bias"].double(),
        cfg.get("order_k", 1), cfg.get("score_heuristic", "greedy"), reduce_none=cfg.get("reduce_red_op", "sum") is None)
    assert torch.equal(mis, c["expected"]["so"]["mis"]) and torch.equal(cluster, c["expected"]["so"]["cluster_index"])
    torch.testing.assert_close(score, f["score"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(x_pool, f["x"], rtol=1e-12, atol=1e-12)


def random_graph(seed, n, p, directed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(n, n, generator=g) < p
    a.fill_diagonal_(False)
    if not directed:
        a = torch.triu(a, 1)
        a = a | a.t()
    return a.nonzero().t().contiguous(), g


@pytest.mark.parametrize("k", [1, 2, 3])
def test_equals_the_sequential_greedy_on_undirected_graphs(k):
    for seed in range(12):
        n = 10 + 5 * seed
        ei, g = random_graph(seed, n, 0.08, directed=False)
        perm = torch.randperm(n, generator=g)
        mis, _ = R.mis_cluster(ei, k, perm, n)
        assert torch.equal(mis, R.sequential_greedy(ei, k, perm, n)), (seed, k)
        mis, _ = R.mis_cluster(ei, k, None, n)
        assert torch.equal(mis, R.sequential_greedy(ei, k, None, n)), (seed, k)


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_results_are_independent_maximal_and_reached(k, directed):
    for seed in range(10):
        n = 12 + 6 * seed
        ei, g = random_graph(100 + seed, n, 0.07, directed)
        perm = torch.randperm(n, generator=g)
        mis, cluster = R.mis_cluster(ei, k, perm, n)
        reach = R.reach_within(ei, k, n)  # reach[i, j]: i reaches j within k hops
        members = mis.nonzero().view(-1)
        sub = reach[members][:, members].clone()
        sub.fill_diagonal_(False)
        if not directed:
            assert not bool(sub.any()), "two members within k hops"
        else:  # a later member may reach an earlier one; never the other way round, and never both ways
            assert not bool((sub & sub.t()).any())
        assert bool(reach[members].any(0).all()), "a node no member reaches"
        assert int(cluster.max()) + 1 == members.numel() and torch.equal(cluster[members], torch.arange(members.numel()))
        assert bool(reach[members[cluster], torch.arange(n)].all()), "a node whose member does not reach it"


def test_ties_go_to_the_lower_index_and_degenerate_inputs():
    ei = torch.tensor([[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2]])  # a path of four nodes, equal scores
    mis, cluster, upd = R.select(torch.ones(4), ei, 1, None, 4)
    assert mis.tolist() == [0, 2] and cluster.tolist() == [0, 0, 1, 1]
    mis, cluster, _ = R.select(torch.ones(5), torch.empty(2, 0, dtype=torch.long), 2, "greedy", 5)
    assert mis.tolist() == [0, 1, 2, 3, 4] and cluster.tolist() == [0, 1, 2, 3, 4]
    mis, cluster = R.mis_cluster(torch.empty(2, 0, dtype=torch.long), 1, None, 0)
    assert mis.numel() == 0 and cluster.numel() == 0
