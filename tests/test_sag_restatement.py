"""The plain-torch restatement of SAGPooling's score, selection and Reduce (tests/sag_restatement.py, the
project-then-aggregate form) against the reference's stored results (tests/golden/golden_sag_v1.pt: cases whose kept and
dropped scores are at least 1e-4 apart and whose float64 run keeps the same nodes), against the aggregate-then-project
formulation of PyG's layers, and on a four-node case checked by hand.  The GPU tests then hold the kernels to it."""
import os

import pytest
import torch

import sag_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_sag_v1.pt"), weights_only=True)["cases"]


def test_fixture_set_covers_what_it_should():
    cfgs = [c["cfg"] for c in CASES.values()]
    assert {c["gnn"] for c in CASES.values()} == {"graphconv", "sage"}
    assert any(c["inputs"]["batch"] is None for c in CASES.values())
    assert any(c.get("aggr") == "mean" for c in cfgs) and any(isinstance(c.get("ratio"), int) for c in cfgs)
    assert any(c.get("min_score") is not None for c in cfgs) and any(c.get("multiplier", 1.0) != 1.0 for c in cfgs)
    assert any(c.get("nonlinearity") == "identity" for c in cfgs) and any(c.get("degree_norm") for c in cfgs)
    assert any(c.get("remove_self_loops") is False for c in cfgs) and any(c.get("connect_red_op") == "max" for c in cfgs)
    attn_dims = {c["inputs"]["attn"].dim() for c in CASES.values() if c["inputs"].get("attn") is not None}
    assert attn_dims == {1, 2}
    directed = [n for n, c in CASES.items() if not torch.equal(
        *(torch.zeros(c["inputs"]["x"].size(0), c["inputs"]["x"].size(0)).index_put_(
            (ei[0], ei[1]), torch.ones(ei.size(1))) for ei in (c["inputs"]["edge_index"], c["inputs"]["edge_index"].flip(0))))]
    assert directed, "no directed edge list among the fixtures"
    unsorted = [n for n, c in CASES.items() if not bool(
        (c["inputs"]["edge_index"][1][1:] >= c["inputs"]["edge_index"][1][:-1]).all())]
    assert unsorted, "no list that needs the by-destination permutation among the fixtures"


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference(name):
    c = CASES[name]
    e = c["expected"]
    raw, score, perm, weight, x_pool = R.pool_case(c)
    node_index, cluster_index = R.assignment(perm)
    torch.testing.assert_close(raw, e["score"], rtol=1e-5, atol=1e-5)
    assert torch.equal(node_index, e["so"]["node_index"]) and torch.equal(cluster_index, e["so"]["cluster_index"]), name
    assert e["so"]["num_supernodes"] == perm.numel() and e["so"]["num_nodes"] == c["inputs"]["x"].size(0)
    torch.testing.assert_close(weight[cluster_index], e["so"]["weight"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(x_pool, e["x"], rtol=1e-5, atol=1e-5)
    if c["inputs"]["batch"] is not None:
        assert torch.equal(c["inputs"]["batch"][perm], e["batch"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_float64_run(name):
    c = CASES[name]
    f = c["f64"]
    x = c["inputs"]["x"].double().requires_grad_(True)
    par = {k: v.double().requires_grad_(True) for k, v in c["params"].items()}
    raw, score, perm, weight, x_pool = R.pool_case(c, torch.float64, params=par, x=x)
    node_index, cluster_index = R.assignment(perm)
    assert torch.equal(node_index, c["expected"]["so"]["node_index"])
    assert torch.equal(cluster_index, c["expected"]["so"]["cluster_index"])
    torch.testing.assert_close(raw, f["score"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(weight[cluster_index], f["weight"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(x_pool, f["x"], rtol=1e-12, atol=1e-12)
    names = sorted(par)
    grads = torch.autograd.grad((x_pool ** 2).sum(), [x] + [par[k] for k in names], allow_unused=True)
    torch.testing.assert_close(grads[0], f["grads"]["x"], rtol=1e-9, atol=1e-12)
    for k, g in zip(names, grads[1:]):
        torch.testing.assert_close(g if g is not None else torch.zeros_like(par[k]), f["grads"]["params"][k],
                                   rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("mean", [False, True])
def test_projection_and_aggregation_commute(mean):
    """lin_rel(aggr_j x_j) + lin_root(x_i), the E x F gather and N x F scatter of the composed form, equals the scalar
    form; duplicates, self-loops and nodes without an incoming edge included."""
    g = torch.Generator().manual_seed(3)
    n, F, E = 40, 7, 300
    x = torch.randn(n, F, generator=g, dtype=torch.float64)
    ei = torch.randint(0, n - 3, (2, E), generator=g)  # the last three nodes have no edge at all
    ei = torch.cat([ei, ei[:, :20], torch.arange(5).repeat(2, 1)], 1)
    rel, root = torch.nn.Linear(F, 1).double(), torch.nn.Linear(F, 1, bias=False).double()
    agg = torch.zeros(n, F, dtype=torch.float64).index_add_(0, ei[1], x[ei[0]])
    if mean:
        agg = agg / torch.bincount(ei[1], minlength=n).clamp(min=1).view(-1, 1)
    want = (rel(agg) + root(x)).view(-1)
    got = R.raw_score(x, ei, rel.weight, root.weight, rel.bias, mean)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_four_nodes_by_hand():
    """x = [1, 2, 3, 4] (one feature), w_rel = 2, w_root = -1, b = 0.5; edges 0->1, 2->1, 1->1 (self-loop), 3->0, 3->0
    (duplicate); node 2 and node 3 have no incoming edge.  p = 2x = [2, 4, 6, 8], q = -x.
    sum:  t = [8+8+0.5-1, 2+6+4+0.5-2, 0.5-3, 0.5-4] = [15.5, 10.5, -2.5, -3.5]
    mean: t = [16/2+0.5-1, 12/3+0.5-2, 0.5-3, 0.5-4] = [7.5, 2.5, -2.5, -3.5]
    ratio 0.5 keeps the two best: nodes 0 and 1."""
    x = torch.tensor([[1.0], [2.0], [3.0], [4.0]])
    ei = torch.tensor([[0, 2, 1, 3, 3], [1, 1, 1, 0, 0]])
    w_rel, w_root, b = torch.tensor([[2.0]]), torch.tensor([[-1.0]]), torch.tensor([0.5])
    assert R.raw_score(x, ei, w_rel, w_root, b, False).tolist() == [15.5, 10.5, -2.5, -3.5]
    assert R.raw_score(x, ei, w_rel, w_root, b, True).tolist() == [7.5, 2.5, -2.5, -3.5]
    raw, score, perm, weight, x_pool = R.pool(x, ei, None, w_rel, w_root, b, nonlinearity="identity")
    assert perm.tolist() == [0, 1] and weight.tolist() == [15.5, 10.5] and x_pool.view(-1).tolist() == [15.5, 21.0]
    perm = R.pool(x, ei, None, -w_rel, -w_root, -b, nonlinearity="identity")[2]  # every score negated: 3 then 2
    assert perm.tolist() == [3, 2] and [t.tolist() for t in R.assignment(perm)] == [[2, 3], [1, 0]]
    batch = torch.tensor([0, 0, 1, 1])
    assert R.select(raw, batch, 0.5).tolist() == [0, 2] and R.select(raw, batch, 1).tolist() == [0, 2]
    assert R.select(raw, batch, 5).tolist() == [0, 1, 2, 3]
    soft = R.activate(raw, batch, min_score=0.9)
    assert R.select(soft, batch, min_score=0.9).tolist() == [0, 2]  # graph 1's best (0.73) is below 0.9: it alone is kept
