"""The HOSC restatement (tests/hosc_restatement.py, which forms A A A explicitly) pinned to the reference's own fixtures
(tests/golden/golden_hosc_v1.pt, made by tests/golden/make_golden_hosc.py), on the CPU:

* float64: losses and every gradient of each loss alone (with respect to x and the selector parameters) within 1e-12 of
  the reference's float64 run.  ``hosc_loss`` relative to itself (a ratio of same-sign sums), ``ortho_loss`` with
  ``hosc_ortho`` relative to mu sqrt(K) / (sqrt(K) - 1) (the larger of its two cancelling terms), otherwise to itself;
  gradients relative to their max-norm.
* float32: losses at rtol = atol = 1e-5 of the reference's float32 outputs.
"""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hosc_restatement as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "golden_hosc_v1.pt")
CASES = torch.load(GOLDEN, weights_only=False)["cases"]
POOL = sorted(k for k, v in CASES.items() if v["kind"] == "pool")
REL64 = 1e-12


def _close64(got, want, scale):
    err = abs(float(got) - float(want))
    assert err <= REL64 * float(scale), (float(got), float(want), err, float(scale))


def ortho_scale(cfg, want):
    k = cfg["k"]
    if cfg.get("hosc_ortho", False) and k > 1 and cfg.get("mu", 0.1) != 0:
        return cfg.get("mu", 0.1) * math.sqrt(k) / (math.sqrt(k) - 1)
    return abs(float(want))


def test_fixture_holds_every_required_case():
    names = set(CASES)
    for mode in ("hosc", "hosc_u"):
        for tag in ("default", "hosc_ortho", "alpha1", "alpha0_mu0", "k1_hosc_ortho", "sparse_out", "noT_ewn", "raw", "mlp2",
                    "unweighted", "single_graph", "edgeless_graph"):
            assert f"{mode}_{tag}" in names, (mode, tag)
    assert {"hosc_dense_inputs_mask", "hosc_dense_inputs_mask_dirty", "hosc_functions_f32", "hosc_functions_f64"} <= names
    assert os.path.getsize(GOLDEN) < 400 * 1024


@pytest.mark.parametrize("name", POOL)
def test_restatement_f64_losses_and_gradients(name):
    case = CASES[name]
    ours = R.pool_grads(case, torch.float64)
    ref = case["f64"]
    for loss in R.LOSSES:
        value, grads = ours[loss]
        want = ref["losses"][loss]
        print(name, loss, float(value), float(want))
        _close64(value, want, ortho_scale(case["cfg"], want) if loss == "ortho_loss" else abs(float(want)))
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
        losses, _, _ = R.pool_losses(case, torch.float32)
    for loss in R.LOSSES:
        torch.testing.assert_close(losses[loss], case["expected"]["loss"][loss], rtol=1e-5, atol=1e-5)


def test_directed_case_separates_the_two_modes():
    """The fixture's directed batch: the batched (A^T: in-degrees) and unbatched (out-degrees) hosc losses differ."""
    b = CASES["hosc_default"]["f64"]["losses"]["hosc_loss"]
    u = CASES["hosc_u_default"]["f64"]["losses"]["hosc_loss"]
    assert abs(float(b) - float(u)) > 1e-6 * max(abs(float(b)), abs(float(u)))


def function_values(i, dtype):
    """The restatement's values of the fixture's function cases (shared with the GPU test's expectations)."""
    s, mask, ei, ew, batch, sf = i["s"], i["mask"], i["edge_index"], i["edge_weight"], i["batch"], i["s_flat"]
    nb = int(batch.max()) + 1
    one = batch[ei[0]] == 0
    a, ptr, sizes = R.dense_blocks(ei, ew, batch, nb, dtype)
    au = R.dense_blocks(ei, torch.ones_like(ew), batch, nb, dtype)[0]
    sp = R.pad_rows(sf, batch, ptr, nb, a.size(1))
    a0 = R.dense_blocks(ei[:, one], ew[one], torch.zeros(6, dtype=torch.long), 1, dtype)[0]
    zero = torch.zeros((), dtype=dtype)
    return {
        "ortho_mask": R.hosc_ortho_terms(s, mask.sum(1)).mean(),
        "ortho_nomask": R.hosc_ortho_terms(s, s.size(1)).mean(),
        "ortho_sum": R.hosc_ortho_terms(s, mask.sum(1)).sum(),
        "ortho_k1": zero,
        "unbatched_ortho": R.hosc_ortho_terms(sp, sizes.to(dtype)).mean(),
        "unbatched_ortho_sum": R.hosc_ortho_terms(sp, sizes.to(dtype)).sum(),
        "unbatched_ortho_nobatch": R.hosc_ortho_terms(sf.unsqueeze(0), sf.size(0)).mean(),
        "unbatched_ortho_k1": zero,
        "ho_w": R.ho_cut_terms(a, sp).mean(),
        "ho_u": R.ho_cut_terms(au, sp).mean(),
        "ho_sum": R.ho_cut_terms(a, sp).sum(),
        "ho_nobatch": R.ho_cut_terms(a0, sf[:6].unsqueeze(0))[0],
        "ho_nobatch_sum": R.ho_cut_terms(a0, sf[:6].unsqueeze(0))[0],
        "ho_no_edges": zero,
        "ho_no_edges_nobatch": zero,
    }


@pytest.mark.parametrize("tag,dtype", [("f32", torch.float32), ("f64", torch.float64)])
def test_restatement_loss_functions(tag, dtype):
    case = CASES[f"hosc_functions_{tag}"]
    e = case["expected"]
    ours = function_values(case["inputs"], dtype)
    assert set(ours) == set(e)
    k = case["inputs"]["s"].size(-1)
    for name, v in ours.items():
        print(name, float(v), float(e[name]))
        assert v.shape == e[name].shape, name
        if dtype == torch.float64:
            scale = math.sqrt(k) / (math.sqrt(k) - 1) * (3 if name.endswith("sum") else 1) if "ortho" in name \
                else abs(float(e[name]))
            _close64(v, e[name], scale)
        else:
            torch.testing.assert_close(v, e[name], rtol=1e-5, atol=1e-5)
