"""The float64-capable restatement of BN-Pool (tests/bnpool_restatement.py) against the reference's own results
(tests/golden/golden_bnpool_v1.pt), on the CPU: the loss functions in float64 at 1e-12, every pooler case (stored stick
fractions and sampled non-edges injected) at the project's fp32 tolerance."""
import os

import pytest
import torch

import bnpool_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_bnpool_v1.pt"), weights_only=True)["cases"]
POOL = sorted(n for n, c in CASES.items() if c["kind"] == "pool")
TOL = 1e-5


def _dense_x(x, batch):
    if x.dim() == 3:
        return x
    if batch is None:
        return x.unsqueeze(0)
    sizes = torch.bincount(batch)
    ptr = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])
    out = x.new_zeros(sizes.numel(), int(sizes.max()), x.size(1))
    out[batch, torch.arange(x.size(0)) - ptr[batch]] = x
    return out


def _selector(c):
    p = c["params"]
    n = len([k for k in p if k.startswith("selector.mlp.lins.") and k.endswith(".weight")])
    ws = [p[f"selector.mlp.lins.{i}.weight"] for i in range(n)]
    bs = [p.get(f"selector.mlp.lins.{i}.bias") for i in range(n)]
    return ws, bs, c["cfg"].get("act")


def restated_case(c, dtype=torch.float32):
    """(S, losses) of a fixture's pooler case from the restatement."""
    i, p, cfg = c["inputs"], c["params"], c["cfg"]
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t  # noqa: E731
    ws, bs, act = _selector(c)
    ws, bs = [cast(w) for w in ws], [None if b is None else cast(b) for b in bs]
    pri = [cast(p[k]) for k in ("alpha_prior", "beta_prior", "K_mu", "K_var")]
    kw = dict(eta=cfg.get("eta", 1.0), train_K=cfg.get("train_K", True))
    z = cast(c["z"])
    if c["alias"].endswith("_u"):
        alpha, beta = R.selector_params(cast(i["x"]), ws, bs, act)
        s = R.sticks_to_s(z)
        batch = i.get("batch")
        nb = 1 if batch is None else int(batch.max()) + 1
        return s, R.sparse_losses(s, cast(p["K"]), i["edge_index"], c["neg_edge_index"], batch, nb, alpha, beta, pri[0],
                                  pri[1], pri[2], pri[3], **kw)
    if "adj" in i:
        x, adj, mask = i["x"], cast(i["adj"]), i.get("mask")
    else:
        x = _dense_x(i["x"], i.get("batch"))
        adj, mask = R.dense_adjacency(i["edge_index"], i.get("edge_weight"), i.get("batch"), i["x"].size(0),
                                      cfg.get("adj_transpose", True), dtype)
    alpha, beta = R.selector_params(cast(x), ws, bs, act)
    s = R.sticks_to_s(z, mask)
    return s, R.bnpool_losses(s, cast(p["K"]), adj, mask, alpha, beta, pri[0], pri[1], pri[2], pri[3], **kw)


@pytest.mark.parametrize("name", POOL)
def test_restatement_reproduces_the_pooler_cases(name):
    c = CASES[name]
    s, losses = restated_case(c)
    want = c["expected"]
    torch.testing.assert_close(s.reshape(want["so"]["s"].shape), want["so"]["s"], rtol=TOL, atol=TOL)
    assert set(losses) == set(want["loss"]) == {"quality", "kl", "K_prior"}
    for k, v in want["loss"].items():
        torch.testing.assert_close(losses[k].float(), v, rtol=TOL, atol=TOL, msg=lambda m: f"{name}/{k}: {m}")


def test_orientation_is_observable():
    """K is asymmetric in the fixtures: the transposed adjacency gives another reconstruction loss."""
    c = CASES["bnpool_default"]
    i = c["inputs"]
    _, good = restated_case(c)
    adj, mask = R.dense_adjacency(i["edge_index"], i["edge_weight"], i["batch"], i["x"].size(0), False)
    s = c["expected"]["so"]["s"]
    flipped = R.rec_terms(s, c["params"]["K"], adj, mask).mean()
    assert abs(float(flipped) - float(good["quality"])) > 1e-3 * abs(float(good["quality"]))


@pytest.mark.parametrize("tag,tol", [("f64", 1e-12), ("f32", 1e-5)])
def test_restated_functions_match_the_reference(tag, tol):
    c = CASES[f"bnpool_functions_{tag}"]
    i, e = c["inputs"], c["expected"]
    n2 = i["mask"].sum(-1) ** 2
    nn = i["adj"].size(-1) ** 2
    got = {
        "rec_mask": (R.rec_terms_from_logits(i["logits"], i["adj"], i["mask"]) / n2).mean(),
        "rec_mask_sum": (R.rec_terms_from_logits(i["logits"], i["adj"], i["mask"]) / n2).sum(),
        "rec_nomask": (R.rec_terms_from_logits(i["logits"], i["adj"]) / nn).mean(),
        "rec_nonorm": R.rec_terms_from_logits(i["logits"], i["adj"], i["mask"]).mean(),
        "rec_unbalanced": (R.rec_terms_from_logits(i["logits"], i["adj"], i["mask"], balance=False) / n2).mean(),
        "rec_pm30": (R.rec_terms_from_logits(i["logits"] * 10, i["adj"], i["mask"]) / n2).mean(),
        "kl_mask": (R.kl_terms(i["alpha"], i["beta"], i["prior_alpha"], i["prior_beta"], i["mask"]) / n2).mean(),
        "kl_nomask": (R.kl_terms(i["alpha"], i["beta"], i["prior_alpha"], i["prior_beta"]) / nn).mean(),
        "prior": R.prior_term(i["K"], i["K_mu"], i["K_var"]),
        "prior_vec": (R.prior_term(i["K"], i["K_mu"], i["K_var"]) / n2.numel() / n2).mean(),
    }
    for k, v in got.items():
        assert abs(float(v) - float(e[k])) <= tol * abs(float(e[k])), (k, float(v), float(e[k]))
    if tag == "f64":
        for key, scale in (("rec_mask", 1.0), ("rec_pm30", 10.0)):
            leaf = (i["logits"] * scale).clone().requires_grad_(True)
            (R.rec_terms_from_logits(leaf, i["adj"], i["mask"]) / n2).mean().backward()
            want = e[f"grad_{key}"]
            assert float((leaf.grad - want).abs().max()) <= 1e-12 * float(want.abs().max()), key
