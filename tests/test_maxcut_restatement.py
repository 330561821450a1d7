"""The plain-torch restatement of MaxCut pooling (tests/maxcut_restatement.py) against the stored runs of the reference:
the reference-shaped form (the delta-GCN matrix as an explicit list) and the collapsed form the kernels use (no matrix,
``n_P`` as a row bound) are the same function -- float32 at 1e-5, float64 at 1e-12, gradients included."""
import os

import pytest
import torch

import maxcut_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_maxcut_v1.pt"), weights_only=True)["cases"]
POOL = ["maxcut_default", "maxcut_single_graph", "maxcut_directed", "maxcut_weighted", "maxcut_directed_weighted",
        "maxcut_loops_duplicates", "maxcut_isolated", "maxcut_no_assign_all", "maxcut_12_layers", "maxcut_delta",
        "maxcut_int_ratio", "maxcut_identity_acts", "maxcut_relu_layers"]
FORMS = pytest.mark.parametrize("collapsed", [False, True], ids=["reference_shaped", "collapsed"])


def test_the_fixture_holds_the_cases_the_tests_name():
    assert sorted(CASES) == sorted(POOL + ["maxcut_empty", "maxcut_leftovers"])
    assert all(CASES[n]["kind"] == "pool" for n in POOL)
    ei = CASES["maxcut_loops_duplicates"]["inputs"]["edge_index"]
    assert bool((ei[0] == ei[1]).any()) and torch.unique(ei, dim=1).size(1) < ei.size(1)
    assert not bool((ei[1][1:] >= ei[1][:-1]).all())  # shuffled: the permutation route
    iso = CASES["maxcut_isolated"]["inputs"]
    assert not bool((iso["edge_index"] == 2).any()) and int(iso["edge_index"].max()) + 2 == iso["x"].size(0)
    assert CASES["maxcut_empty"]["inputs"]["edge_index"].size(1) == 0
    assert CASES["maxcut_single_graph"]["inputs"]["batch"] is None
    assert len(CASES["maxcut_12_layers"]["cfg"]["mp_units"]) == 12 and CASES["maxcut_delta"]["cfg"]["delta"] != 2
    assert CASES["maxcut_int_ratio"]["cfg"]["ratio"] == 3
    directed = CASES["maxcut_directed"]["inputs"]["edge_index"]
    assert not torch.equal(torch.unique(directed, dim=1), torch.unique(directed.flip(0), dim=1))
    for n in POOL:  # the contract of a top-k: kept and dropped scores apart, kept scores pairwise apart
        e, b = CASES[n]["expected"], CASES[n]["inputs"]["batch"]
        s = e["scores"]
        b = b if b is not None else torch.zeros(s.numel(), dtype=torch.long)
        kept = torch.zeros(s.numel(), dtype=torch.bool)
        kept[e["kept"]] = True
        for g in range(int(b.max()) + 1):
            k, d = s[(b == g) & kept], s[(b == g) & ~kept]
            assert not d.numel() or float(k.min() - d.max()) >= 1e-4
            assert k.numel() < 2 or float(k.sort().values.diff().min()) >= 1e-4


@FORMS
@pytest.mark.parametrize("name", POOL)
def test_float32_reproduces_the_reference(name, collapsed):
    c = CASES[name]
    e = c["expected"]
    got = R.pool_case(c, collapsed=collapsed)
    torch.testing.assert_close(got["scores"], e["scores"], rtol=1e-5, atol=1e-5)
    assert torch.equal(got["kept"], e["kept"])
    if c["cfg"].get("assign_all_nodes", True):
        assert torch.equal(got["cluster_index"], e["cluster_index"])
    torch.testing.assert_close(got["x_pool"], e["x"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got["loss"], e["loss"]["maxcut_loss"], rtol=1e-5, atol=1e-5)


@FORMS
@pytest.mark.parametrize("name", POOL)
def test_float64_reproduces_the_reference_with_gradients(name, collapsed):
    c = CASES[name]
    f = c["f64"]
    names = f["grads"]["names"]
    par = {k: v.double().requires_grad_(True) for k, v in c["params"].items()}
    x = c["inputs"]["x"].double().requires_grad_(True)
    got = R.pool_case(c, torch.float64, collapsed=collapsed, params=par, x=x, kept=c["expected"]["kept"])
    torch.testing.assert_close(got["scores"], f["scores"], rtol=1e-12, atol=1e-12)
    assert torch.equal(R.select(got["scores"], c["inputs"]["batch"], c["cfg"].get("ratio", 0.5)), f["kept"])
    torch.testing.assert_close(got["x_pool"], f["x"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got["loss"], f["loss"]["maxcut_loss"], rtol=1e-12, atol=1e-12)
    grads = torch.autograd.grad((got["x_pool"] ** 2).sum() + got["loss"], [x] + [par[k] for k in names], allow_unused=True)
    torch.testing.assert_close(grads[0], f["grads"]["x"], rtol=1e-11, atol=1e-12)
    flat = torch.cat([(torch.zeros_like(par[k]) if g is None else g).reshape(-1) for k, g in zip(names, grads[1:])])
    torch.testing.assert_close(flat, f["grads"]["params_flat"], rtol=1e-11, atol=1e-12)


@FORMS
def test_an_empty_edge_list_scores_every_node_alike(collapsed):
    c = CASES["maxcut_empty"]
    got = R.pool_case(c, collapsed=collapsed, kept=torch.zeros(1, dtype=torch.long))
    torch.testing.assert_close(got["scores"], c["expected"]["scores"], rtol=1e-5, atol=1e-5)
    assert float(got["scores"].max() - got["scores"].min()) == 0.0  # act(b) everywhere: no row of P exists
    assert float(got["loss"]) == 0.0 and float(c["expected"]["loss"]["maxcut_loss"]) == 0.0
    got64 = R.pool_case(c, torch.float64, collapsed=collapsed, kept=torch.zeros(1, dtype=torch.long))
    torch.testing.assert_close(got64["scores"], c["f64"]["scores"], rtol=1e-12, atol=1e-12)


def test_trailing_nodes_get_no_diagonal_term():
    """n_P is the list's largest endpoint + 1: a node above it gets act(b), an isolated node below it (1 - delta) z."""
    z = torch.tensor([[1.0], [2.0], [4.0], [8.0]])
    ei = torch.tensor([[0, 2], [2, 0]])
    w = torch.ones(2)
    h = R.layer_collapsed(z, ei, w, R.dinv_of(ei, w, 4), R.n_p_of(ei), 2.0, torch.tensor([0.5]))
    assert h.view(-1).tolist() == [-1.0 + 8.0 + 0.5, -2.0 + 0.5, -4.0 + 2.0 + 0.5, 0.5]


def test_the_assignment_breaks_ties_to_the_lowest_label_and_counts_duplicates():
    kept = torch.tensor([0, 1])
    assert R.assign_rounds(kept, torch.tensor([[1, 0], [2, 2]]), 3, 1) == [1, 2, 1]  # one vote each
    assert R.assign_rounds(kept, torch.tensor([[0, 1, 1], [2, 2, 2]]), 3, 1) == [1, 2, 2]  # a duplicate decides
    chain = torch.tensor([[0, 2], [2, 3]])
    assert R.assign_rounds(torch.tensor([0]), chain, 4, 1) == [1, 0, 1, 0]  # a round reads the labels of its start
    assert R.assign_rounds(torch.tensor([0]), chain, 4, 2) == [1, 0, 1, 1]
