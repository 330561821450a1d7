"""A torch restatement of Just Balance pooling's auxiliary loss (reference poolers/just_balance.py,
utils/losses.py:553-594, 1013-1080) in this project's own words, for float32 and float64 on any device.

Per graph with assignment S (its rows: ALL N rows of a padded batch, masked ones included; the rows of the graph in an
un-padded batch):
    c_k = sum_i S_ik^2,   L = -sum_k sqrt(c_k + eps),   normalised: L / sqrt(n K)
n = mask.sum() (padded with a mask), ``num_nodes`` or N (padded without), the graph's rows (un-padded); K =
``num_supernodes`` or the columns of S.  Only the diagonal of S^T S enters, so only it is computed: a plain loop over
the graphs.  The batch reduction is a mean or a sum.

Used as the oracle of tests/test_jb_restatement.py (pinned to the reference's fixtures) and tests/test_gpu_jb.py.
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import tgp_oracle as O  # noqa: E402

EPS = 1e-8
LOSSES = ("balance_loss",)


def _seg_sum(src, index, size):
    return src.new_zeros((size,) + tuple(src.shape[1:])).index_add_(0, index, src)


def graph_term(S, n, k=None, normalize=True):
    """One graph: S [rows, K] -> -sum_k sqrt(sum_i S_ik^2 + eps), over sqrt(n k) when normalised."""
    k = S.size(1) if k is None else k
    loss = -torch.sqrt((S * S).sum(0) + EPS).sum()
    if normalize:
        loss = loss / math.sqrt(n * k) if n > 0 else loss / torch.zeros((), dtype=S.dtype, device=S.device)
    return loss


def dense_terms(S, mask=None, normalize=True, num_nodes=None, num_supernodes=None):
    """[B] per-graph terms of a padded batch S [B,N,K]."""
    out = []
    for b in range(S.size(0)):
        n = int(mask[b].sum()) if mask is not None else (S.size(1) if num_nodes is None else num_nodes)
        out.append(graph_term(S[b], n, num_supernodes, normalize))
    return torch.stack(out)


def flat_terms(S, batch=None, normalize=True):
    """[B] per-graph terms of an un-padded batch S [Ntot,K] (``batch`` None: one graph)."""
    if batch is None:
        return graph_term(S, S.size(0), None, normalize).unsqueeze(0)
    out = []
    for g in range(int(batch.max()) + 1):
        rows = S[batch == g]
        out.append(graph_term(rows, rows.size(0), None, normalize))
    return torch.stack(out)


def selector(params, dtype):
    """(weights, biases) of MLPSelect's Linear layers from a state dict, as leaves of the given dtype."""
    idx = sorted({int(k.split(".")[3]) for k in params if k.startswith("selector.mlp.lins.")})
    ws = [params[f"selector.mlp.lins.{i}.weight"].to(dtype).clone().requires_grad_(True) for i in idx]
    bs = [params[f"selector.mlp.lins.{i}.bias"].to(dtype).clone().requires_grad_(True) for i in idx]
    names = [f"selector.mlp.lins.{i}.{p}" for i in idx for p in ("weight", "bias")]
    return ws, bs, names


def pool_losses(case, dtype, device="cpu", weights=None, biases=None, x=None):
    """(losses, S, {"x_pool", "adj_pool"}) of a fixture case (``cfg``, ``inputs``, ``params``): the loss with its
    coefficient, S, and the pooled features and (post-processed, oracle) adjacency.  ``weights`` / ``biases`` / ``x``:
    leaves to differentiate."""
    cfg, inp = case["cfg"], case["inputs"]
    batched = case["alias"] == "jb"
    if weights is None:
        weights, biases, _ = selector(case["params"], dtype)
    if x is None:
        x = inp["x"].to(dtype)
    x = x.to(device)
    weights = [w.to(device) for w in weights]
    biases = [b.to(device) for b in biases]
    act = cfg.get("act")
    normalize = cfg.get("normalize_loss", True)
    if "adj" in inp:  # already dense
        a = inp["adj"].to(dtype).to(device)
        mask = inp.get("mask")
        mask = (torch.ones(x.shape[:2], dtype=torch.bool) if mask is None else mask).to(device)
        xd = x
    else:
        ei = inp["edge_index"].to(device)
        w = inp.get("edge_weight")
        w = (torch.ones(ei.size(1), dtype=dtype) if w is None else w.to(dtype)).to(device)
        batch = inp.get("batch")
    if batched:
        if "adj" not in inp:
            bt = batch if batch is not None else torch.zeros(x.size(0), dtype=torch.long)
            xd, a, mask = O.dense_preprocessing(x.cpu(), ei.cpu(), w.cpu(), bt.cpu(), cfg.get("adj_transpose", True))
            xd, a, mask = xd.to(device), a.to(device), mask.to(device)
        s = O.mlp_select(xd, weights, biases, mask, act)
        terms = dense_terms(s, mask, normalize)
        raw = s.transpose(1, 2) @ a @ s
        x_pool = s.transpose(1, 2) @ xd
    else:
        s = O.mlp_select(x, weights, biases, None, act)
        bt = batch.to(device) if batch is not None else torch.zeros(x.size(0), dtype=torch.long, device=device)
        nb = int(bt.max()) + 1
        terms = flat_terms(s, bt, normalize)
        raw = torch.zeros(nb, s.size(1), s.size(1), dtype=s.dtype, device=device).index_add_(
            0, bt[ei[0]], w.view(-1, 1, 1) * s[ei[0]].unsqueeze(2) * s[ei[1]].unsqueeze(1))
        x_pool = _seg_sum(s.unsqueeze(2) * x.unsqueeze(1), bt, nb)
    losses = {"balance_loss": terms.mean() * cfg.get("loss_coeff", 1.0)}
    adj_pool = O.postprocess_dense(raw, cfg.get("remove_self_loops", True), cfg.get("degree_norm", True),
                                   cfg.get("adj_transpose", True) if batched else False, cfg.get("edge_weight_norm", False))
    return losses, s, {"x_pool": x_pool, "adj_pool": adj_pool}


def pool_grads(case, dtype, device="cpu"):
    """{loss: (value, {"x": dL/dx, "params": {name: dL/dp}})} of the restatement."""
    weights, biases, names = selector(case["params"], dtype)
    x = case["inputs"]["x"].to(dtype).clone().requires_grad_(True)
    losses, _, _ = pool_losses(case, dtype, device, weights, biases, x)
    leaves = [x] + [t for pair in zip(weights, biases) for t in pair]
    out = {}
    for n in LOSSES:
        g = torch.autograd.grad(losses[n], leaves, retain_graph=True, allow_unused=True)
        g = [torch.zeros_like(l) if gi is None else gi for gi, l in zip(g, leaves)]
        out[n] = (losses[n].detach(), {"x": g[0], "params": dict(zip(names, g[1:]))})
    return out
