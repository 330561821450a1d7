"""The Just Balance restatement (tests/jb_restatement.py) pinned to the reference's own fixtures
(tests/golden/golden_jb_v1.pt, made by tests/golden/make_golden_jb.py), on the CPU:

* float64: the loss and every gradient of it (with respect to x and the selector parameters) within 1e-12 of the
  reference's float64 run; the loss relative to its magnitude (a sum of terms of one sign), gradients relative to their
  max-norm.
* float32: the loss at rtol = atol = 1e-5 of the reference's float32 output.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jb_restatement as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "golden_jb_v1.pt")
CASES = torch.load(GOLDEN, weights_only=False)["cases"]
POOL = sorted(k for k, v in CASES.items() if v["kind"] == "pool")
REL64 = 1e-12
TAGS = ("default", "sparse_out", "noT_ewn", "raw", "mlp2", "nonorm", "coeff05")


def _close64(got, want, scale):
    err = abs(float(got) - float(want))
    assert err <= REL64 * float(scale), (float(got), float(want), err, float(scale))


def test_fixture_holds_every_required_case():
    names = set(CASES)
    for mode in ("batched", "unbatched"):
        for tag in TAGS:
            assert {f"jb_{mode}_{tag}_w", f"jb_{mode}_{tag}_u"} <= names
    assert {"jb_single_graph", "jb_u_single_graph", "jb_dense_inputs_mask", "jb_dense_inputs_mask_dirty_x",
            "jb_dense_inputs_nomask", "jb_functions_f32", "jb_functions_f64"} <= names
    assert os.path.getsize(GOLDEN) < 1 << 20
    i = CASES["jb_functions_f32"]["inputs"]
    assert bool((i["s"][:, :, 2] == 0).all()) and bool((i["s_flat"][:, 1] == 0).all())  # a zero column each
    assert bool((i["s"][~i["mask"]] == 0).all()) and bool((i["s_dirty"][~i["mask"]] != 0).any())
    # (the value the reference gives for the default weighted batch, both modes of the pooler agreeing on the formula)
    assert abs(float(CASES["jb_batched_default_w"]["expected"]["loss"]["balance_loss"]) + 0.5203) < 5e-5


@pytest.mark.parametrize("name", POOL)
def test_restatement_f64_loss_and_gradients(name):
    case = CASES[name]
    ours = R.pool_grads(case, torch.float64)
    ref = case["f64"]
    for loss in R.LOSSES:
        value, grads = ours[loss]
        want = ref["losses"][loss]
        print(name, loss, float(value), float(want))
        _close64(value, want, abs(float(want)))
        pairs = [(grads["x"], ref["grads"][loss]["x"])]
        pairs += [(grads["params"][n], ref["grads"][loss]["params"][n]) for n in grads["params"]]
        for g, gr in pairs:
            top = float(gr.abs().max()) if gr.numel() else 0.0
            err = float((g - gr).abs().max()) if gr.numel() else 0.0
            print("  grad", loss, tuple(gr.shape), err, top)
            assert err <= REL64 * top, (loss, err, top)


@pytest.mark.parametrize("name", POOL)
def test_restatement_f32_loss(name):
    case = CASES[name]
    with torch.no_grad():
        losses, _, _ = R.pool_losses(case, torch.float32)
    for loss in R.LOSSES:
        torch.testing.assert_close(losses[loss], case["expected"]["loss"][loss], rtol=1e-5, atol=1e-5)


def function_values(i, dense_terms, flat_terms):
    """The fixture's "functions" entries from per-graph term functions with the restatement's signatures (shared with
    the API and GPU tests, which pass the product's own)."""
    s, sd, mask, batch, sf = i["s"], i["s_dirty"], i["mask"], i["batch"], i["s_flat"]
    return {
        "mask": dense_terms(s, mask).mean(),
        "nomask": dense_terms(s).mean(),
        "dirty_mask": dense_terms(sd, mask).mean(),
        "dirty_nomask": dense_terms(sd).mean(),
        "mask_nonorm": dense_terms(s, mask, normalize=False).mean(),
        "mask_sum": dense_terms(s, mask).sum(),
        "dirty_mask_sum": dense_terms(sd, mask).sum(),
        "nomask_n5_k6": dense_terms(s, num_nodes=5, num_supernodes=6).mean(),
        "mask_n5_k6": dense_terms(s, mask, num_nodes=5, num_supernodes=6).mean(),
        "unbatched": flat_terms(sf, batch).mean(),
        "unbatched_nobatch": flat_terms(sf).mean(),
        "unbatched_nonorm": flat_terms(sf, batch, normalize=False).mean(),
        "unbatched_sum": flat_terms(sf, batch).sum(),
    }


@pytest.mark.parametrize("tag,dtype", [("f32", torch.float32), ("f64", torch.float64)])
def test_restatement_loss_functions(tag, dtype):
    case = CASES[f"jb_functions_{tag}"]
    e = case["expected"]
    ours = function_values(case["inputs"], R.dense_terms, R.flat_terms)
    assert set(ours) == set(e)
    for k, v in ours.items():
        print(k, float(v), float(e[k]))
        assert v.dtype == dtype
        if dtype == torch.float64:
            _close64(v, e[k], abs(float(e[k])))
        else:
            torch.testing.assert_close(v, e[k], rtol=1e-5, atol=1e-5)
