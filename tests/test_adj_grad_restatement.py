"""The closed form of the dense poolers' adjacency gradient (tests/adj_grad_restatement.py) against the float64 autograd
of the oracle (oracle/tgp_oracle.py: dense_pool, mincut_loss, link_pred_loss), on the CPU: every differentiable output
is sent back alone with a fixed random upstream gradient, and dA of the closed form must agree with autograd's within
1e-10 relative (the float64 bound of tests/test_gpu_grad_paths.py).  A path that does not reach A has no gradient there."""
import itertools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adj_grad_restatement as R  # noqa: E402

F64_BOUND = 1e-10  # (test_gpu_grad_paths.F64_BOUND: float64 against the float64 oracle)

CONFIGS = [dict(alias=alias, adj_transpose=at, remove_self_loops=rsl, degree_norm=dn, normalize_loss=nl)
           for alias, at, (rsl, dn), nl in itertools.product(("mincut", "diff"), (False, True),
                                                              itertools.product((False, True), repeat=2), (False, True))
           if alias == "diff" or not nl]  # (normalize_loss is DiffPool's)


def _id(c):
    return "-".join([c["alias"], "at" if c["adj_transpose"] else "noat", "rsl" if c["remove_self_loops"] else "sl",
                     "dn" if c["degree_norm"] else "nodn"] + (["norm"] if c["normalize_loss"] else []))


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=[_id(c) for c in CONFIGS])
def test_closed_form_matches_float64_autograd(cfg, masked):
    cfg = dict(cfg)
    alias = cfg.pop("alias")
    if alias == "mincut":
        cfg.pop("normalize_loss")
    B, N, K, F = 3, 9, 4, 5
    x, adj, mask, ws, bs = R.make_inputs(B, N, K, F, seed=11 + masked, sizes=[9, 1, 6] if masked else None)
    assert not torch.equal(adj, adj.transpose(1, 2))
    outs, _, _ = R.oracle_run(alias, x, adj, mask, ws, bs, torch.float64, **cfg)
    reached = set()
    for pi, path in enumerate(outs):
        g = torch.Generator().manual_seed(100 + pi)
        up = torch.randn(outs[path].shape, generator=g, dtype=torch.float64)
        o, lv, s = R.oracle_run(alias, x, adj, mask, ws, bs, torch.float64, **cfg)
        (want,) = torch.autograd.grad(o[path], [lv["adj"]], up, allow_unused=True)
        s, a = s.detach(), lv["adj"].detach()
        g_r = g_cut = g_link = None
        scale = 1.0
        if path == "adj":
            raw = s.transpose(1, 2) @ a @ s
            g_r = R.post_backward(raw, up, cfg["remove_self_loops"], cfg["degree_norm"], cfg["adj_transpose"])
        elif path.endswith("cut_loss"):
            g_cut = (up / B).expand(B)
        elif path.endswith("link_loss"):
            g_link = up
            scale = 1.0 / a.numel() if cfg["normalize_loss"] else 1.0
        else:  # pooled features, orthogonality, entropy: A is not in them
            assert want is None or not bool(want.abs().max() > 0), path
            continue
        got = R.adj_grad(s, a, g_r, g_cut, g_link, scale)
        assert want is not None and bool(want.abs().max() > 0), path
        err = float(torch.linalg.vector_norm(got - want)) / float(torch.linalg.vector_norm(want))
        assert err <= F64_BOUND, (path, err)
        assert float((got - want).abs().max()) <= 4 * F64_BOUND * float(want.abs().max()), path
        reached.add(path.split(":")[-1])
    assert reached == ({"adj", "cut_loss"} if alias == "mincut" else {"adj", "link_loss"})


def test_zero_link_norm_takes_the_subgradient():
    """A = S S^T exactly: torch.norm's gradient at 0 is 0, and so is c."""
    s = torch.softmax(torch.randn(2, 5, 3, dtype=torch.float64), -1)
    a = s @ s.transpose(1, 2)
    m, gamma, c = R.coefficients(s, a, None, None, torch.tensor(1.0, dtype=torch.float64), 1.0)
    assert float(c) == 0.0 and not bool(m.abs().max() > 0) and not bool(gamma.abs().max() > 0)
