"""The ACC restatement (tests/acc_restatement.py) and the package's own float64 composed loss forms, both pinned to the
reference's fixtures (tests/golden/golden_acc_v1.pt, made by tests/golden/make_golden_acc.py), on the CPU:

* float64: losses and every gradient of each loss alone (with respect to x and the selector parameters) within 1e-12 of
  the reference's float64 run.  The total variation (a sum of non-negative terms) relative to its magnitude, the balance
  loss relative to the larger of its magnitude and its coefficient (it is 1 - sum / beta: the two terms cancel),
  gradients relative to their max-norm.
* float32: losses at rtol = atol = 1e-5 of the reference's float32 outputs.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import acc_restatement as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "golden_acc_v1.pt")
CASES = torch.load(GOLDEN, weights_only=False)["cases"]
POOL = sorted(k for k, v in CASES.items() if v["kind"] == "pool")
REL64 = 1e-12


class Package:
    """The package's public loss functions in the shape acc_restatement.pool_losses asks for (float64 on the host: the
    composed torch forms)."""

    @staticmethod
    def totvar(adj, S):
        from tgp.utils.losses import totvar_loss
        return totvar_loss(S, adj, batch_reduction="mean").reshape(1)

    @staticmethod
    def asym(S, k, mask=None):
        from tgp.utils.losses import asym_norm_loss
        return asym_norm_loss(S, k, mask=mask, batch_reduction="mean").reshape(1)

    @staticmethod
    def sparse_totvar(edge_index, S, w, batch, nb):
        from tgp.utils.losses import sparse_totvar_loss
        return sparse_totvar_loss(edge_index, S, w, batch, batch_reduction="mean").reshape(1)

    @staticmethod
    def unbatched_asym(S, k, batch, nb):
        from tgp.utils.losses import unbatched_asym_norm_loss
        return unbatched_asym_norm_loss(S, k, batch, batch_reduction="mean").reshape(1)


def _scale(loss, want, cfg):
    if loss == "balance_loss":
        return max(abs(float(want)), abs(cfg.get("balance_coeff", 1.0)))
    return abs(float(want))


def _close64(got, want, scale):
    err = abs(float(got) - float(want))
    assert err <= REL64 * float(scale), (float(got), float(want), err, float(scale))


def test_fixture_holds_every_required_case():
    names = set(CASES)
    for tag in ("default", "sparse_out", "noT_ewn", "coeffs", "mlp2"):
        assert {f"acc_batched_{tag}_w", f"acc_batched_{tag}_u"} <= names
    assert {"acc_single_graph", "acc_u_single_graph", "acc_dense_inputs_mask", "acc_dense_inputs_nomask",
            "acc_directed_w", "acc_u_directed_w", "acc_directed_noT_w", "acc_edgeless_graph_w", "acc_u_edgeless_graph_w",
            "acc_zero_weight_edges", "acc_u_zero_weight_edges", "acc_k1", "acc_u_k1", "acc_n_lt_k", "acc_u_n_lt_k",
            "acc_functions_f32", "acc_functions_f64"} <= names
    assert any(k.startswith("acc_unbatched_") for k in names)
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("forms", [R.Restated, Package], ids=["restatement", "package"])
@pytest.mark.parametrize("name", POOL)
def test_f64_losses_and_gradients(name, forms):
    case = CASES[name]
    ours = R.pool_grads(case, torch.float64, forms=forms)
    ref = case["f64"]
    for loss in R.LOSSES:
        value, grads = ours[loss]
        want = ref["losses"][loss]
        print(name, loss, float(value), float(want))
        _close64(value, want, _scale(loss, want, case["cfg"]))
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


def test_the_two_forms_count_edges_differently():
    """Zero-weight edges: the edge form counts them, the dense form (nonzero entries) does not."""
    b = CASES["acc_zero_weight_edges"]["f64"]["losses"]["total_variation_loss"]
    u = CASES["acc_u_zero_weight_edges"]["f64"]["losses"]["total_variation_loss"]
    assert abs(float(b) - float(u)) > 1e-3 * max(abs(float(b)), abs(float(u)))


def function_values(forms, i, nb):
    """The twelve stored function cases from per-graph forms (``forms`` as acc_restatement.Restated)."""
    a, s, mask = i["adj"], i["s"], i["mask"]
    ei, ew, batch, sf = i["edge_index"], i["edge_weight"], i["batch"], i["s_flat"]
    one = batch[ei[0]] == 0
    zeros = torch.zeros(sf.size(0), dtype=torch.long, device=sf.device)
    k = s.size(-1)
    return {
        "totvar": forms.totvar(a, s).mean(),
        "totvar_sum": forms.totvar(a, s).sum(),
        "sparse_totvar_w": forms.sparse_totvar(ei, sf, ew, batch, nb).mean(),
        "sparse_totvar_u": forms.sparse_totvar(ei, sf, None, batch, nb).mean(),
        "sparse_totvar_nobatch": forms.sparse_totvar(ei[:, one], sf[:6], ew[one], zeros[:6], 1).mean(),
        "asym_mask": forms.asym(s, k, mask).mean(),
        "asym_sum": forms.asym(s, k, mask).sum(),
        "asym_k1": forms.asym(s, 1).mean(),
        "asym_k9": forms.asym(s[:, :5], 9, mask[:, :5]).mean(),
        "asym_nomask": forms.asym(s[:, :4], k).mean(),
        "unbatched_asym": forms.unbatched_asym(sf, k, batch, nb).mean(),
        "unbatched_asym_nobatch": forms.unbatched_asym(sf, k, zeros, 1).mean(),
        "unbatched_asym_k2": forms.unbatched_asym(sf, 2, batch, nb).mean(),
    }


@pytest.mark.parametrize("tag,dtype", [("f32", torch.float32), ("f64", torch.float64)])
def test_restatement_loss_functions(tag, dtype):
    case = CASES[f"acc_functions_{tag}"]
    i, e = case["inputs"], case["expected"]
    ours = function_values(R.Restated, i, int(i["batch"].max()) + 1)
    assert set(ours) == set(e)
    for k, v in ours.items():
        print(k, float(v), float(e[k]))
        if dtype == torch.float64:
            _close64(v, e[k], max(abs(float(e[k])), 1.0) if "asym" in k else abs(float(e[k])))
        else:
            torch.testing.assert_close(v, e[k], rtol=1e-5, atol=1e-5)
