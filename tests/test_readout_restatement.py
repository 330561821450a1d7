"""The plain-torch restatement of the readout against every case the reference produced (``golden_readout_v1.pt``):
the float32 and the float64 results, the pooled batch vector, and the float64 gradients of ``sum(out ** 2)``."""
import pytest
import torch

import readout_restatement as R

CASES = R.load_cases()


def test_the_fixture_holds_every_route_and_operation():
    assert len(CASES) == 50
    assert {c["op"] for c in CASES.values()} == {"sum", "mean", "max", "min", "multi"}
    assert any("mask" in c["inputs"] for c in CASES.values()) and any("node_index" in c["inputs"] for c in CASES.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_reference(name):
    c = CASES[name]
    out, bp, _ = R.run_case(c)
    e = c["expected"]
    assert out.shape == e["x"].shape
    if c["op"] in ("max", "min"):
        assert torch.equal(out, e["x"])
    torch.testing.assert_close(out, e["x"], rtol=1e-5, atol=1e-5)
    if e["batch"] is None:
        assert bp is None
    else:
        assert torch.equal(bp, e["batch"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_reference_in_float64_with_gradients(name):
    c = CASES[name]
    out, _, leaves = R.run_case(c, torch.float64, grad=True)
    torch.testing.assert_close(out, c["f64"]["x"], rtol=1e-13, atol=1e-13)
    grads = torch.autograd.grad((out ** 2).sum(), leaves)
    torch.testing.assert_close(grads[0], c["f64"]["grads"]["x"], rtol=1e-12, atol=1e-12)
    if "weight" in c["f64"]["grads"]:
        torch.testing.assert_close(grads[1], c["f64"]["grads"]["weight"], rtol=1e-12, atol=1e-12)


def test_empty_groups_and_mean_denominator():
    x = torch.tensor([[1.0, -2.0], [3.0, 4.0], [5.0, 6.0]])
    index = torch.tensor([0, 0, 3])
    for op, want in (("sum", [[4, 2], [0, 0], [0, 0], [5, 6]]), ("mean", [[2, 1], [0, 0], [0, 0], [5, 6]]),
                     ("max", [[3, 4], [0, 0], [0, 0], [5, 6]]), ("min", [[1, -2], [0, 0], [0, 0], [5, 6]])):
        assert torch.equal(R.scatter(x, index, 4, op), torch.tensor(want, dtype=torch.float32)), op
