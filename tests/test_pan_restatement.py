"""The PAN restatement (tests/pan_restatement.py) on the CPU: against the fixture the reference's ``PANPooling`` made, the
structural-pattern rule, ``deg`` as a count, the cumulative-product coefficients -- and the package's composed form
(``tgp.nn.pan_met_composed``), which must give the restatement's pattern in the restatement's order."""
import os

import pytest
import torch

import pan_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_pan_v1.pt"), weights_only=True)["cases"]
TOL = dict(rtol=1e-5, atol=1e-5)


def restated(c, dtype=torch.float32, leaves=None, perm=None):
    i, cfg = c["inputs"], c["cfg"]
    x_in, w, lw, lb, p, beta = leaves if leaves is not None else (
        [i["x"].to(dtype)] + [c["conv"][k].to(dtype) for k in ("weight", "lin.weight", "lin.bias")]
        + [c["params"][k].to(dtype) for k in ("p", "beta")])
    x, index, values = R.conv(x_in, i["edge_index"], w, lw, lb, i["batch"])
    return (x, index, values) + R.pool(x, index, values, i["batch"], p, beta, cfg.get("nonlinearity", "tanh"),
                                       cfg.get("ratio", 0.5), cfg.get("min_score"), cfg.get("multiplier", 1.0), perm)


def test_the_fixture_covers_the_cases_of_the_issue():
    assert sorted(c["filter_size"] for c in CASES.values() if c["filter_size"] != 2) == [1, 3, 4]
    assert CASES["pan_single_graph"]["inputs"]["batch"] is None
    ei = CASES["pan_loops_and_duplicates"]["inputs"]["edge_index"]
    assert bool((ei[0] == ei[1]).any()) and torch.unique(ei, dim=1).size(1) < ei.size(1)
    b, ei = CASES["pan_edgeless_graph"]["inputs"]["batch"], CASES["pan_edgeless_graph"]["inputs"]["edge_index"]
    assert not bool((b[ei[0]] == 2).any()) and int((b == 2).sum()) > 0
    ei = CASES["pan_directed_batch"]["inputs"]["edge_index"]
    assert not torch.equal(torch.unique(ei, dim=1), torch.unique(ei.flip(0), dim=1))
    cfgs = [c["cfg"] for c in CASES.values()]
    for key, value in (("min_score", 0.05), ("ratio", 3), ("multiplier", 2.0), ("degree_norm", True),
                       ("connect_red_op", "max"), ("nonlinearity", "identity")):
        assert any(cfg.get(key) == value for cfg in cfgs), key


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_fixture(name):
    c = CASES[name]
    e = c["expected"]
    x, index, values, raw, score, perm, weight, x_pool, p_index, p_values = restated(c)
    assert torch.equal(index, e["met_index"])
    torch.testing.assert_close(values, e["met_values"], **TOL)
    torch.testing.assert_close(x, e["conv_out"], **TOL)
    torch.testing.assert_close(score, e["score"], **TOL)
    node_index, order = torch.sort(perm)
    assert torch.equal(node_index, e["so"]["node_index"]) and torch.equal(order, e["so"]["cluster_index"])
    torch.testing.assert_close(x_pool, e["x"], **TOL)
    assert e["edge_weight"] is None and e["edge_index"]["__coo__"]
    assert e["edge_index"]["size"] == [perm.numel(), perm.numel()]
    # the pooled matrix: the induced submatrix in the input's order, relabelled in ascending node order
    assert torch.equal(p_index, e["edge_index"]["indices"])
    if not c["cfg"].get("degree_norm"):
        torch.testing.assert_close(p_values, e["edge_index"]["values"], **TOL)


@pytest.mark.parametrize("name", ["pan_undirected_batch", "pan_directed_batch", "pan_identity", "pan_filter_4"])
def test_restatement_gradients_match_the_fixture(name):
    c = CASES[name]
    f = c["f64"]
    i = c["inputs"]
    leaves = [i["x"].double()] + [c["conv"][k].double() for k in ("weight", "lin.weight", "lin.bias")] + [
        c["params"][k].double() for k in ("p", "beta")]
    leaves = [v.clone().requires_grad_(True) for v in leaves]
    node_index, order = c["expected"]["so"]["node_index"], c["expected"]["so"]["cluster_index"]
    perm = torch.empty_like(node_index)
    perm[order] = node_index
    out = restated(c, torch.float64, leaves, perm)
    torch.testing.assert_close(out[0], f["conv_out"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(out[7], f["x"], rtol=1e-12, atol=1e-12)
    g = torch.autograd.grad((out[7] ** 2).sum(), leaves)
    want = [f["grads"]["x"]] + [f["grads"]["conv"][k] for k in ("weight", "lin.weight", "lin.bias")] + [
        f["grads"]["params"][k] for k in ("p", "beta")]
    for got, w in zip(g, want):
        torch.testing.assert_close(got, w, rtol=1e-10, atol=1e-12)


def path(n):
    return torch.stack([torch.arange(n - 1), torch.arange(1, n)])  # 0 -> 1 -> ... -> n - 1


def test_the_pattern_is_structural_with_a_zero_and_a_negative_weight():
    """A zero weight removes every later term's value, a negative one can cancel: the entries stay."""
    ei = torch.tensor([[0, 1, 2, 0], [1, 2, 0, 2]])  # a triangle 0 -> 1 -> 2 -> 0 and the chord 0 -> 2
    n = 3
    idx_ref, _ = R.met(ei, torch.ones(3, dtype=torch.float64), n)
    for w in ([0.5, 0.0, 0.7], [1.0, 1.0, -1.0], [0.0, 0.0, 0.0]):
        idx, val = R.met(ei, torch.tensor(w, dtype=torch.float64), n)
        assert torch.equal(idx, idx_ref), w
    # 2's row: walks into 2 of length <= 2 start at 2, 1, 0 (0 -> 2 and 0 -> 1 -> 2: the terms of c_1 and c_2 meet)
    idx, val = R.met(ei, torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64), n)
    dense = torch.zeros(n, n, dtype=torch.float64).index_put((idx[0], idx[1]), val)
    stored = torch.zeros(n, n, dtype=torch.bool).index_put((idx[0], idx[1]), torch.ones(idx.size(1), dtype=torch.bool))
    assert bool(stored[2, 0]) and float(dense[2, 0]) == 0.0  # c_1 * 1 + c_2 * 1 = 1 - 1: stored, and zero
    idx, val = R.met(ei, torch.tensor([0.0, 0.0, 0.0], dtype=torch.float64), n)
    assert idx.size(1) == idx_ref.size(1) and float(val.abs().max()) == 0.0
    assert bool(stored.diagonal().all())


def test_deg_counts_stored_entries():
    """Duplicate edges change S, not deg; dinv is deg^-1/2 of the count."""
    ei = torch.tensor([[0, 0, 0, 1], [1, 1, 1, 2]])  # 0 -> 1 three times, 1 -> 2
    w = torch.tensor([1.0, 1.0], dtype=torch.float64)
    m, pattern, s, deg = R.met_dense_one(ei, w, 4)
    assert deg.tolist() == [1.0, 2.0, 2.0, 1.0]  # node 3 is isolated: its diagonal alone
    assert float(s[1, 0]) == 3.0  # the multiplicity is in S
    assert float(m[1, 0]) == pytest.approx(3.0 / (1.0 ** 0.5 * 2.0 ** 0.5))
    assert float(m[3, 3]) == 1.0 and float(m[0, 0]) == 1.0


def test_coefficients_are_cumulative_products():
    ei = path(5)
    w = torch.tensor([0.9, 0.5, -2.0, 0.25], dtype=torch.float64)
    _, pattern, s, _ = R.met_dense_one(ei, w, 5)
    c = torch.cumprod(w, 0)
    a = R.transposed_adjacency(ei, 5, torch.float64)
    want = sum(c[k] * torch.linalg.matrix_power(a, k) for k in range(4))
    torch.testing.assert_close(s, want, rtol=1e-14, atol=0)
    # the path 0 -> ... -> 4: row i holds i, i - 1, ... down to i - 3
    assert pattern.sum(1).tolist() == [1, 2, 3, 4, 4]
    assert float(s[4, 1]) == float(c[3]) and float(s[4, 0]) == 0.0 and not bool(pattern[4, 0])


def test_an_edgeless_graph_gives_weight0_times_identity():
    idx, val = R.met(torch.zeros(2, 0, dtype=torch.long), torch.tensor([0.3, 0.5, 0.5], dtype=torch.float64), 4)
    assert torch.equal(idx, torch.arange(4).repeat(2, 1)) and val.tolist() == [0.3] * 4


@pytest.mark.parametrize("name", sorted(CASES))
def test_composed_form_gives_the_restatements_pattern_order_and_values(name):
    from tgp.nn import pan_met_composed
    c = CASES[name]
    i = c["inputs"]
    w = c["conv"]["weight"].double().requires_grad_(True)
    idx, val = pan_met_composed(i["edge_index"], w, i["x"].size(0))
    w2 = c["conv"]["weight"].double().requires_grad_(True)
    idx_ref, val_ref = R.met(i["edge_index"], w2, i["x"].size(0), i["batch"])
    assert torch.equal(idx, idx_ref)
    torch.testing.assert_close(val, val_ref, rtol=1e-13, atol=1e-15)
    g = torch.randn(val.numel(), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    torch.testing.assert_close(torch.autograd.grad((val * g).sum(), w)[0], torch.autograd.grad((val_ref * g).sum(), w2)[0],
                               rtol=1e-11, atol=1e-13)


def test_composed_form_keeps_the_pattern_under_zero_weights_and_cross_graph_edges():
    from tgp.nn import pan_met_composed
    ei = torch.tensor([[0, 1, 2, 0, 3], [1, 2, 0, 2, 0]])  # 3 -> 0 joins what a batch vector [0, 0, 0, 1] would split
    for w in ([0.5, 0.0, 0.7], [1.0, 1.0, -1.0]):
        wt = torch.tensor(w, dtype=torch.float64)
        idx, val = pan_met_composed(ei, wt, 4)
        idx_ref, val_ref = R.met(ei, wt, 4)
        assert torch.equal(idx, idx_ref)
        torch.testing.assert_close(val, val_ref, rtol=1e-13, atol=1e-15)
