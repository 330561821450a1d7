"""The GTVConv restatement (tests/gtv_restatement.py) on the CPU: against the fixture the reference's ``GTVConv.forward``
made (outputs and gradients in float64), the cases the fixture must hold, and the package's composed form
(``tgp.mp.gtv_propagate_composed``), which must equal the restatement bit for bit."""
import os

import pytest
import torch

import gtv_restatement as R
from test_gpu_grad_paths import FACTOR, FLOOR

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_gtv_v1.pt"), weights_only=True)["cases"]


def connectivity(c, dtype, grad=False):
    """(second argument of the layer, edge weights, the leaf holding the edge values or None) of a fixture case."""
    i = c["inputs"]
    if "adj" in i:
        adj = i["adj"].to(dtype).clone().requires_grad_(grad)
        return adj, None, adj
    w = i.get("edge_weight")
    if w is not None:
        w = w.to(dtype).clone().requires_grad_(grad)
    return i["edge_index"], w, w


def restated(c, dtype, grad=False):
    cfg, i = c["cfg"], c["inputs"]
    x = i["x"].to(dtype).clone().requires_grad_(grad)
    weight = c["params"]["weight"].to(dtype).clone().requires_grad_(grad)
    bias = c["params"].get("bias")
    if bias is not None:
        bias = bias.to(dtype).clone().requires_grad_(grad)
    conn, w, edge_leaf = connectivity(c, dtype, grad)
    out = R.layer(x, weight, bias, conn, w, i.get("mask"), cfg.get("delta_coeff", 1.0), cfg.get("eps", 1e-3), cfg["act"])
    leaves = {"x": x, "weight": weight, "bias": bias, ("adj" if "adj" in i else "edge_weight"): edge_leaf}
    return out, {k: v for k, v in leaves.items() if v is not None}


def test_the_fixture_covers_the_cases_of_the_issue():
    cfgs = [c["cfg"] for c in CASES.values()]
    assert {cfg["act"] for cfg in cfgs} == {"identity", "relu", "elu", "tanh"}
    assert {cfg.get("delta_coeff", 1.0) for cfg in cfgs} == {0.311, 1.0}
    assert {cfg.get("eps", 1e-3) for cfg in cfgs} == {1e-3, 0.5}
    assert any(cfg.get("bias") is False for cfg in cfgs)
    assert CASES["gtv_undirected_unweighted"]["inputs"]["edge_weight"] is None
    assert CASES["gtv_undirected_weighted"]["inputs"]["edge_weight"] is not None
    ei = CASES["gtv_directed_elu_delta"]["inputs"]["edge_index"]
    assert not torch.equal(torch.unique(ei, dim=1), torch.unique(ei.flip(0), dim=1))
    ei = CASES["gtv_loops_duplicates_unsorted"]["inputs"]["edge_index"]
    assert bool((ei[0] == ei[1]).any()) and torch.unique(ei, dim=1).size(1) < ei.size(1)
    assert not bool((ei[0, 1:] >= ei[0, :-1]).all())
    i = CASES["gtv_isolated_nodes_tanh"]["inputs"]
    assert torch.unique(i["edge_index"]).numel() <= i["x"].size(0) - 3
    c = CASES["gtv_zero_distance"]
    h = c["inputs"]["x"] @ c["params"]["weight"]
    assert c["inputs"]["edge_index"][:, 0].tolist() == [0, 1] and torch.equal(h[0], h[1])
    assert CASES["gtv_one_node"]["inputs"]["x"].size(0) == 1
    assert CASES["gtv_edgeless"]["inputs"]["edge_index"].size(1) == 0 and CASES["gtv_edgeless"]["inputs"]["x"].size(0) > 1
    c = CASES["gtv_eps_half"]
    _, d = R.distances(c["inputs"]["x"] @ c["params"]["weight"], c["inputs"]["edge_index"])
    assert float((d < 0.5).float().mean()) > 0.5  # most edges clamped
    assert CASES["gtv_coo_adjacency"]["inputs"]["coo"] is True
    i = CASES["gtv_dense_batch_mask"]["inputs"]
    assert tuple(i["adj"].shape) == (3, 9, 9) and bool((i["adj"].diagonal(dim1=1, dim2=2) != 0).any())
    assert i["mask"].dtype == torch.bool and not bool(i["mask"].all())
    i = CASES["gtv_dense_2d"]["inputs"]
    assert i["adj"].dim() == 2 and i["x"].dim() == 2
    assert os.path.getsize(os.path.join(HERE, "golden", "golden_gtv_v1.pt")) < 300 * 1024


def test_the_fixture_keeps_the_kinks_away_from_float32_noise():
    for name, c in CASES.items():
        i = c["inputs"]
        h = i["x"].double() @ c["params"]["weight"].double()
        if "adj" in i:
            ei, _ = R.dense_edges(i["adj"] if i["adj"].dim() == 3 else i["adj"].unsqueeze(0))
            h = h.reshape(-1, h.size(-1))
        else:
            ei = i["edge_index"]
        diff, d = R.distances(h, ei)
        eps = c["cfg"].get("eps", 1e-3)
        assert not bool(((diff > 0) & (diff < 1e-4)).any()), name
        assert not bool(((d - eps).abs() < 1e-4 * eps).any()), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_fixture_in_float64(name):
    c = CASES[name]
    out, _ = restated(c, torch.float64)
    assert out.shape == c["f64"]["out"].shape
    torch.testing.assert_close(out, c["f64"]["out"], rtol=1e-12, atol=1e-12)
    # in float32 it stays within the float32 reference's own error (which cancels a_ii / eps and gamma h_i - gamma h_i)
    out32, _ = restated(c, torch.float32)
    e = float(torch.linalg.vector_norm(out32.double() - c["f64"]["out"])) / float(torch.linalg.vector_norm(c["f64"]["out"]))
    assert e <= max(FACTOR * c["e_ref32"], FLOOR), (name, e, c["e_ref32"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gradients_match_the_fixture(name):
    c = CASES[name]
    out, leaves = restated(c, torch.float64, grad=True)
    got = torch.autograd.grad(out, list(leaves.values()), c["f64"]["upstream"], allow_unused=True)
    assert set(leaves) == set(c["f64"]["grads"])
    for (leaf, v), g in zip(leaves.items(), got):
        want = c["f64"]["grads"][leaf]
        g = torch.zeros_like(v) if g is None else g
        if leaf == "adj":  # the reference's matrix form gives zero entries a gradient too; the edge form only the others
            nz = c["inputs"]["adj"] != 0
            off = ~torch.eye(nz.size(-1), dtype=torch.bool).expand_as(nz)
            g, want = g[nz & off], want[nz & off]
        scale = max(float(want.abs().max()), 1e-300) if want.numel() else 1.0
        torch.testing.assert_close(g, want, rtol=1e-10, atol=1e-12 * max(scale, 1.0), msg=lambda m: f"{name}/{leaf}: {m}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_composed_form_equals_the_restatement_bit_for_bit(name):
    from tgp.mp import gtv_propagate_composed
    c = CASES[name]
    cfg, i = c["cfg"], c["inputs"]
    h = i["x"].double() @ c["params"]["weight"].double()
    bias = c["params"].get("bias")
    bias = None if bias is None else bias.double()
    mask = None
    if "adj" in i:
        adj = (i["adj"] if i["adj"].dim() == 3 else i["adj"].unsqueeze(0)).double()
        ei, w = R.dense_edges(adj)
        h = h.reshape(-1, h.size(-1))
        mask = None if i.get("mask") is None else i["mask"].reshape(-1)
    else:
        ei, w = i["edge_index"], (None if i["edge_weight"] is None else i["edge_weight"].double())
    act = R.ACTS[cfg["act"]]
    args = (bias, mask, cfg.get("delta_coeff", 1.0), cfg.get("eps", 1e-3), act)
    assert torch.equal(gtv_propagate_composed(h, ei, w, *args), R.propagate(h, ei, w, *args))


def test_self_loops_drop_out_duplicates_add_and_the_sum_lands_at_the_source():
    h = torch.tensor([[0.0, 0.0], [1.0, 2.0], [4.0, -1.0]], dtype=torch.float64)
    # 0 <- 1 once: node 0 moves towards node 1 by delta * (h_1 - h_0) / d, d = 3; node 1 and 2 have no out-edge
    out = R.propagate(h, torch.tensor([[0], [1]]), delta=0.5)
    torch.testing.assert_close(out, h + torch.tensor([[0.5 / 3, 1.0 / 3], [0, 0], [0, 0]], dtype=torch.float64))
    twice = R.propagate(h, torch.tensor([[0, 0, 2, 1], [1, 1, 2, 1]]), delta=0.5)
    torch.testing.assert_close(twice, h + torch.tensor([[1.0 / 3, 2.0 / 3], [0, 0], [0, 0]], dtype=torch.float64))
    # an end outside [0, N) leaves the edge out
    assert torch.equal(R.propagate(h, torch.tensor([[0, 0, -1], [1, 3, 1]]), delta=0.5), out)


def test_a_clamped_edge_uses_eps_and_a_zero_distance_edge_has_an_exact_zero_gradient():
    h = torch.tensor([[0.0, 0.0], [0.1, 0.1], [0.0, 0.0]], dtype=torch.float64, requires_grad=True)
    w = torch.tensor([2.0, 3.0], dtype=torch.float64, requires_grad=True)
    out = R.propagate(h, torch.tensor([[0, 0], [1, 2]]), w, eps=0.5)  # d = 0.2 < eps, and d = 0
    torch.testing.assert_close(out[0], 2.0 / 0.5 * h[1].detach())
    gh, gw = torch.autograd.grad(out[0].sum(), [h, w])
    assert float(gw[1]) == 0.0 and bool(torch.isfinite(gh).all())
    torch.testing.assert_close(gw[0], torch.tensor(0.2 / 0.5, dtype=torch.float64))
