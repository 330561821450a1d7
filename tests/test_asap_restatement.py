"""The plain-torch restatement of ASAP pooling (tests/asap_restatement.py) against the stored runs of the reference: the
reference-shaped form and the collapsed form (no ``F x F`` Linear per row, LEConv as three projections) are the same
function -- float32 at 1e-5, float64 at 1e-12, gradients included."""
import os

import pytest
import torch

import asap_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_asap_v1.pt"), weights_only=True)["cases"]
WANTED = ["asap_undirected", "asap_directed", "asap_single_graph", "asap_weighted", "asap_self_loops_unsorted",
          "asap_duplicates", "asap_isolated", "asap_int_ratio", "asap_tanh", "asap_slope_zero", "asap_keep_self_loops",
          "asap_degree_norm", "asap_connect_max", "asap_gnn", "asap_one_column"]


def test_the_fixture_holds_the_cases_the_tests_name():
    assert sorted(CASES) == sorted(WANTED)
    c = CASES["asap_duplicates"]["inputs"]["edge_index"]
    assert torch.unique(c, dim=1).size(1) < c.size(1)
    loops = CASES["asap_self_loops_unsorted"]["inputs"]["edge_index"]
    assert bool((loops[0] == loops[1]).any()) and not bool((loops[0][1:] >= loops[0][:-1]).all())
    iso = CASES["asap_isolated"]["inputs"]["edge_index"]
    assert not bool((iso == 2).any())
    assert CASES["asap_single_graph"]["inputs"]["batch"] is None and CASES["asap_one_column"]["inputs"]["x"].dim() == 1
    for c in CASES.values():  # no two sources tie in a master query: the arg-max is a contract
        x = c["inputs"]["x"]
        assert torch.unique(x.view(x.size(0), -1), dim=0).size(0) == x.size(0)


@pytest.mark.parametrize("collapsed", [False, True], ids=["reference_shaped", "collapsed"])
@pytest.mark.parametrize("name", WANTED)
def test_float32_reproduces_the_reference(name, collapsed):
    c = CASES[name]
    e = c["expected"]
    got = R.pool_case(c, collapsed=collapsed)
    for key, want in (("alpha", e["alpha"]), ("x_new", e["x_new"]), ("fitness", e["score"]), ("x_pool", e["x"])):
        torch.testing.assert_close(got[key], want, rtol=1e-5, atol=1e-5, msg=lambda m, k=key: f"{name} {k}: {m}")
    node_index, cluster_index = R.assignment(got["perm"])
    assert torch.equal(node_index, e["so"]["node_index"]) and torch.equal(cluster_index, e["so"]["cluster_index"])
    torch.testing.assert_close(got["weight"][cluster_index], e["so"]["weight"], rtol=1e-5, atol=1e-5)
    assert torch.equal(got["batch"][got["perm"]], e["batch"])


@pytest.mark.parametrize("collapsed", [False, True], ids=["reference_shaped", "collapsed"])
@pytest.mark.parametrize("name", WANTED)
def test_float64_reproduces_the_reference_with_gradients(name, collapsed):
    c = CASES[name]
    f = c["f64"]
    par = {k: v.double().requires_grad_(True) for k, v in c["params"].items()}
    x = c["inputs"]["x"].double().requires_grad_(True)
    got = R.pool_case(c, torch.float64, collapsed=collapsed, params=par, x=x)
    for key, want in (("alpha", f["alpha"]), ("x_new", f["x_new"]), ("fitness", f["score"]), ("x_pool", f["x"])):
        torch.testing.assert_close(got[key], want, rtol=1e-12, atol=1e-12, msg=lambda m, k=key: f"{name} {k}: {m}")
    assert torch.equal(R.assignment(got["perm"])[0], c["expected"]["so"]["node_index"])
    names = sorted(par)
    grads = torch.autograd.grad((got["x_pool"] ** 2).sum(), [x] + [par[k] for k in names], allow_unused=True)
    torch.testing.assert_close(grads[0], f["grads"]["x"], rtol=1e-12, atol=1e-12)
    for k, g in zip(names, grads[1:]):
        g = torch.zeros_like(par[k]) if g is None else g
        torch.testing.assert_close(g, f["grads"]["params"][k], rtol=1e-12, atol=1e-12, msg=lambda m, k=k: f"{name} {k}: {m}")


def test_the_master_query_reports_the_lowest_position_on_a_tie():
    x = torch.tensor([[1.0, 5.0], [3.0, 5.0], [3.0, 2.0], [0.0, 0.0]])
    ei = torch.tensor([[2, 1, 0, 1, 3], [3, 3, 3, 3, 3]])  # node 3: sources 2, 1, 0, 1 (a duplicate) and itself
    mx, arg = R.master_query(x, ei, 4)
    assert mx[3].tolist() == [3.0, 5.0] and arg[3].tolist() == [0, 1]
    assert arg[0].tolist() == [5, 5]  # no in-edge: one past the list


def test_add_remaining_self_loops_keeps_the_last_loop_weight():
    ei = torch.tensor([[0, 1, 1, 2, 1], [1, 1, 0, 2, 1]])
    ew = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0])
    out, w = R.add_remaining_self_loops(ei, ew, 4)
    assert out.tolist() == [[0, 1, 0, 1, 2, 3], [1, 0, 0, 1, 2, 3]] and w.tolist() == [1.0, 3.0, 1.0, 5.0, 4.0, 1.0]
