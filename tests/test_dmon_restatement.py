"""The DMoN restatement (tests/dmon_restatement.py) pinned to the reference's own fixtures (tests/golden/golden_dmon_v1.pt,
made by tests/golden/make_golden_dmon.py), on the CPU:

* float64: losses and every gradient of each loss alone (with respect to x and the selector parameters) within 1e-12 of
  the reference's float64 run.  Losses relative to their magnitude, the spectral loss relative to trace(raw) / 2m (the
  larger of its two cancelling terms), gradients relative to their max-norm.
* float32: losses at rtol = atol = 1e-5 of the reference's float32 outputs.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dmon_restatement as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "golden_dmon_v1.pt")
CASES = torch.load(GOLDEN, weights_only=False)["cases"]
POOL = sorted(k for k, v in CASES.items() if v["kind"] == "pool")
REL64 = 1e-12


def _close64(got, want, scale):
    err = abs(float(got) - float(want))
    assert err <= REL64 * float(scale), (float(got), float(want), err, float(scale))


def test_fixture_holds_every_required_case():
    names = set(CASES)
    for tag in ("default", "sparse_out", "noT_ewn", "raw", "mlp2"):
        assert {f"dmon_batched_{tag}_w", f"dmon_batched_{tag}_u"} <= names
    assert {"dmon_batched_ortho1_w", "dmon_single_graph", "dmon_u_single_graph", "dmon_dense_inputs_mask",
            "dmon_directed_w", "dmon_u_directed_w", "dmon_edgeless_graph_w", "dmon_u_edgeless_graph_w",
            "dmon_functions_f32", "dmon_functions_f64"} <= names
    assert any(k.startswith("dmon_unbatched_") for k in names)
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", POOL)
def test_restatement_f64_losses_and_gradients(name):
    case = CASES[name]
    ours, scale = R.pool_grads(case, torch.float64)
    ref = case["f64"]
    for loss in R.LOSSES:
        value, grads = ours[loss]
        want = ref["losses"][loss]
        print(name, loss, float(value), float(want))
        _close64(value, want, scale if loss == "spectral_loss" else abs(float(want)))
        pairs = [(grads["x"], ref["grads"][loss]["x"])]
        pairs += [(grads["params"][n], ref["grads"][loss]["params"][n]) for n in grads["params"]]
        for g, gr in pairs:
            top = float(gr.abs().max()) if gr.numel() else 0.0
            err = float((g - gr).abs().max()) if gr.numel() else 0.0
            print("  grad", loss, tuple(gr.shape), err, top)
            assert err <= REL64 * top, (loss, err, top)


@pytest.mark.parametrize("name", POOL)
def test_restatement_f32_losses(name):
    case = CASES[name]
    with torch.no_grad():
        losses, _, _, _ = R.pool_losses(case, torch.float32)
    for loss in R.LOSSES:
        torch.testing.assert_close(losses[loss], case["expected"]["loss"][loss], rtol=1e-5, atol=1e-5)


def test_directed_case_separates_the_two_modes():
    """The fixture's directed batch: the batched (in-degree) and unbatched (out-degree) spectral losses differ."""
    b = CASES["dmon_directed_w"]["f64"]["losses"]["spectral_loss"]
    u = CASES["dmon_u_directed_w"]["f64"]["losses"]["spectral_loss"]
    assert abs(float(b) - float(u)) > 1e-6 * max(abs(float(b)), abs(float(u)))


@pytest.mark.parametrize("tag,dtype", [("f32", torch.float32), ("f64", torch.float64)])
def test_restatement_loss_functions(tag, dtype):
    case = CASES[f"dmon_functions_{tag}"]
    i, e = case["inputs"], case["expected"]
    a, s, raw, mask = i["adj"], i["s"], i["raw"], i["mask"]
    ei, ew, batch, sf = i["edge_index"], i["edge_weight"], i["batch"], i["s_flat"]
    nb = int(batch.max()) + 1
    one = batch[ei[0]] == 0
    spec = {
        "spectral_mask": R.spectral_terms(a, s, raw, mask),
        "spectral_nomask": R.spectral_terms(a, s, raw),
        "sparse_spectral_w": R.sparse_spectral_terms(ei, sf, ew, batch, nb),
        "sparse_spectral_u": R.sparse_spectral_terms(ei, sf, torch.ones_like(ew), batch, nb),
        "sparse_spectral_nobatch": R.sparse_spectral_terms(ei[:, one], sf[:6], ew[one], torch.zeros(6, dtype=torch.long),
                                                           1),
    }
    ours = {k: v[0].mean() for k, v in spec.items()}
    scales = {k: v[1].mean() for k, v in spec.items()}
    ours.update({
        "cluster_mask": R.cluster_terms(s, mask).mean(),
        "cluster_nomask": R.cluster_terms(s).mean(),
        "cluster_sum": R.cluster_terms(s, mask).sum(),
        "unbatched_cluster": R.unbatched_cluster_terms(sf, batch, nb).mean(),
        "unbatched_cluster_nobatch": R.unbatched_cluster_terms(sf, torch.zeros(sf.size(0), dtype=torch.long), 1).mean(),
    })
    assert set(ours) == set(e)
    for k, v in ours.items():
        print(k, float(v), float(e[k]))
        if dtype == torch.float64:
            _close64(v, e[k], scales[k] if k in scales else abs(float(e[k])))
        else:
            torch.testing.assert_close(v, e[k], rtol=1e-5, atol=1e-5)
