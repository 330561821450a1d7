"""The plain-torch restatement of edge-contraction selection (tests/edgepool_restatement.py, ties to the lower edge
position) against the reference's stored results (tests/golden/golden_edgepool_v1.pt: cases whose order the reference's
own unstable ``argsort`` resolved like a stable one), against the reference's formulation of the scores, against a
sequential greedy walk, and on a five-node case checked by hand.  The GPU tests then hold the kernels to this
restatement bit for bit."""
import os

import pytest
import torch

import edgepool_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_edgepool_v1.pt"), weights_only=True)["cases"]
W, B = "selector.lin.weight", "selector.lin.bias"


def run(c, dtype, perm=None):
    i, cfg = c["inputs"], c["cfg"]
    return R.pool(i["x"].to(dtype), i["edge_index"], c["params"][W].to(dtype), c["params"][B].to(dtype), c["method"],
                  cfg.get("add_to_edge_score", 0.5), perm=perm)


def test_fixture_set_covers_what_it_should():
    methods = {c["method"] for c in CASES.values()}
    assert methods == set(R.METHODS)
    assert any(c["inputs"]["batch"] is None for c in CASES.values()) and any(
        c["inputs"]["batch"] is not None for c in CASES.values())
    assert any(c["inputs"]["edge_weight"] is None for c in CASES.values())
    assert {c["cfg"].get("connect_red_op", "sum") for c in CASES.values()} >= {"sum", "max"}
    assert any(c["cfg"].get("degree_norm") for c in CASES.values())
    directed = [n for n, c in CASES.items() if not torch.equal(
        *(torch.zeros(c["inputs"]["x"].size(0), c["inputs"]["x"].size(0)).index_put_(
            (ei[0], ei[1]), torch.ones(ei.size(1))) for ei in (c["inputs"]["edge_index"], c["inputs"]["edge_index"].flip(0))))]
    assert directed, "no directed edge list among the fixtures"


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference(name):
    c = CASES[name]
    e = c["expected"]
    n = c["inputs"]["x"].size(0)
    score, match, cluster, weight, x_pool = run(c, torch.float32)
    torch.testing.assert_close(score, e["score"], rtol=1e-5, atol=1e-5)
    # the stored order is the stable one of the stored scores, and rounding of this magnitude cannot reorder it
    assert torch.equal(R.stable_perm(score), R.stable_perm(e["score"])), name
    assert torch.equal(cluster, e["so"]["cluster_index"]), name
    assert e["so"]["num_supernodes"] == int(cluster.max()) + 1 and e["so"]["num_nodes"] == n
    torch.testing.assert_close(weight, e["so"]["weight"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(x_pool, e["x"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_float64_run(name):
    c = CASES[name]
    f = c["f64"]
    i = c["inputs"]
    x = i["x"].double().requires_grad_(True)
    w = c["params"][W].double().requires_grad_(True)
    b = c["params"][B].double().requires_grad_(True)
    score, match, cluster, weight, x_pool = R.pool(x, i["edge_index"], w, b, c["method"],
                                                   c["cfg"].get("add_to_edge_score", 0.5))
    assert torch.equal(cluster, c["expected"]["so"]["cluster_index"])
    torch.testing.assert_close(score, f["score"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(weight, f["weight"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(x_pool, f["x"], rtol=1e-12, atol=1e-12)
    gx, gw, gb = torch.autograd.grad((x_pool ** 2).sum(), [x, w, b])
    torch.testing.assert_close(gx, f["grads"]["x"], rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(gw, f["grads"]["params"][W], rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(gb, f["grads"]["params"][B], rtol=1e-9, atol=1e-12)


def test_scores_equal_the_reference_formulation():
    """x[row].w1 + x[col].w2 + b is lin(cat([x[row], x[col]])); the softmax is PyG's."""
    g = torch.Generator().manual_seed(5)
    n, F, E = 30, 6, 200
    x = torch.randn(n, F, generator=g, dtype=torch.float64)
    ei = torch.randint(0, n, (2, E), generator=g)
    lin = torch.nn.Linear(2 * F, 1).double()
    raw_ref = lin(torch.cat([x[ei[0]], x[ei[1]]], dim=-1)).view(-1)
    raw = R.raw_scores(x, ei, lin.weight, lin.bias)
    torch.testing.assert_close(raw, raw_ref, rtol=1e-12, atol=1e-12)
    sm = R.normalize(raw, ei, n, "softmax", 0.5)
    for c in range(n):
        sel = ei[1] == c
        if sel.any():
            torch.testing.assert_close(sm[sel], torch.softmax(raw[sel], 0) + 0.5, rtol=1e-12, atol=1e-12)
    # a target with one incoming entry scores exactly 1 + add
    indeg = torch.bincount(ei[1], minlength=n)
    one = indeg[ei[1]] == 1
    if one.any():
        assert bool((R.normalize(raw.float(), ei, n, "softmax", 0.5)[one] == 1.5).all())


def test_five_nodes_by_hand():
    """Entries (position: source -> target, score):
        0: 3 -> 1  0.90      1: 1 -> 3  0.90      2: 2 -> 2  0.95
        3: 0 -> 4  0.50      4: 4 -> 0  0.50      5: 1 -> 2  0.60
    Stable descending order: 2, 0, 1, 5, 3, 4 (the ties 0/1 and 3/4 go to the lower position).  Round 1: entry 2 is the
    minimum at node 2 twice (a self-loop matches its node with itself), entry 0 is the minimum at 3 and at 1 (it beats its
    mirror 1 only by position), entry 3 at 0 and 4; entry 5 touches the matched nodes 1 and 2 and dies.  Representatives:
    cluster[1] = 3 (the source, the LARGER index), cluster[2] = 2, cluster[4] = 0, so rep = [0, 3, 2, 3, 0] and the ids,
    ranks among {0, 2, 3}, are [0, 2, 1, 2, 0].  Had the tie gone to entry 1, rep would be [0, 1, 2, 1, 0]."""
    ei = torch.tensor([[3, 1, 2, 0, 4, 1], [1, 3, 2, 4, 0, 2]])
    e = torch.tensor([0.90, 0.90, 0.95, 0.50, 0.50, 0.60])
    assert R.stable_perm(e).tolist() == [2, 0, 1, 5, 3, 4]
    match, rounds = R.matching(ei, 5, R.stable_perm(e), return_rounds=True)
    assert match.tolist() == [True, False, True, True, False, False] and rounds == 1
    m, cluster, k, weight = R.select(e, ei, 5)
    assert torch.equal(m, match) and k == 3
    assert cluster.tolist() == [0, 2, 1, 2, 0]
    assert weight.tolist() == pytest.approx([0.50, 0.90, 0.95, 0.90, 0.50])
    assert torch.equal(R.sequential_greedy(ei, 5, R.stable_perm(e)), match)


def test_path_with_monotone_scores_takes_half_its_nodes_in_rounds():
    n = 130
    a = torch.arange(n - 1)
    ei = torch.stack([a, a + 1])
    e = torch.linspace(1.0, 0.0, n - 1)
    match, rounds = R.matching(ei, n, R.stable_perm(e), return_rounds=True)
    assert rounds == 65 and int(match.sum()) == 65 and bool(match[0::2].all()) and not bool(match[1::2].any())


@pytest.mark.parametrize("seed", range(8))
def test_rounds_equal_the_sequential_greedy_walk(seed):
    """Directed lists with duplicates and self-loops, a random priority order: the parallel rounds give the matching of
    the sequential walk, which is a valid maximal matching."""
    g = torch.Generator().manual_seed(seed)
    n = int(torch.randint(1, 60, (1,), generator=g))
    E = int(torch.randint(0, 5 * n + 1, (1,), generator=g))
    ei = torch.randint(0, n, (2, E), generator=g)
    perm = torch.randperm(E, generator=g) if seed % 2 else None
    match = R.matching(ei, n, perm)
    assert torch.equal(match, R.sequential_greedy(ei, n, perm))
    touched = torch.zeros(n, dtype=torch.long)
    rows, cols = ei[0][match], ei[1][match]
    touched.index_add_(0, rows, torch.ones_like(rows))
    off = rows != cols
    touched.index_add_(0, cols[off], torch.ones_like(cols[off]))
    assert int(touched.max()) <= 1 if n and E else True  # no node in two matched entries
    assert bool((touched[ei[0]] + touched[ei[1]] > 0).all())  # every entry touches a matched node
    cluster, k = R.clusters(ei, n, match)
    rep = torch.arange(n)
    rep[cols] = rows
    assert torch.equal(cluster, torch.unique(rep, return_inverse=True)[1]) and k == torch.unique(rep).numel()
