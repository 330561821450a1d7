"""A torch restatement of DMoN pooling's three auxiliary losses (reference poolers/dmon.py, utils/losses.py:59-70,
435-473, 1083-1265) in this project's own words, for float32 and float64 on any device.

Batched form, per graph b of a padded batch (A the densified adjacency, A^T when adj_transpose; S masked):
    d = (A 1) * mask,  2m = sum_i d_i,  ca = S^T d,  cs = S^T 1,  n = mask.sum()
    spectral = -(trace(S^T A S) - ||ca||^2 / 2m) / 2m   (0 when m = 0)
    cluster  = ||cs|| sqrt(K) / n - 1
    ortho    = || S^T S / ||S^T S|| - I / sqrt(K) ||
Unbatched form, per graph g of an edge list: d = out-degrees, trace over the graph's edges of w (S_src . S_dst),
m clamped to eps, n = the graph's node count.  Each form returns the batch mean.

Used as the oracle of tests/test_dmon_restatement.py (pinned to the reference's fixtures) and tests/test_gpu_dmon.py.
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import tgp_oracle as O  # noqa: E402

EPS = 1e-8
LOSSES = ("spectral_loss", "cluster_loss", "ortho_loss")


def _seg_sum(src, index, size):
    return src.new_zeros((size,) + tuple(src.shape[1:])).index_add_(0, index, src)


def spectral_terms(adj, S, raw, mask=None):
    """(per-graph spectral loss [B], per-graph |trace(raw)| / 2m [B]: the larger of its two cancelling terms)."""
    if mask is None:
        mask = torch.ones(S.shape[:2], dtype=torch.bool, device=S.device)
    d = adj.sum(-1) * mask
    m2 = d.sum(-1)
    safe = torch.where(m2 > 0, m2, torch.ones_like(m2))
    ca = torch.einsum("bnk,bn->bk", S, d)
    tr = torch.diagonal(raw, dim1=-2, dim2=-1).sum(-1)
    loss = -(tr - (ca * ca).sum(-1) / safe) / safe
    zero = torch.zeros_like(loss)
    return torch.where(m2 > 0, loss, zero), torch.where(m2 > 0, tr.abs() / safe, zero)


def cluster_terms(S, mask=None, k=None):
    k = S.size(-1) if k is None else k
    n = S.size(1) if mask is None else mask.sum(1).to(S.dtype)
    return S.sum(1).norm(dim=-1) / n * math.sqrt(k) - 1


def ortho_terms(S):
    g = S.transpose(1, 2) @ S
    k = S.size(-1)
    eye = torch.eye(k, dtype=S.dtype, device=S.device) / math.sqrt(k)
    return (g / g.norm(dim=(-2, -1), keepdim=True) - eye).norm(dim=(-2, -1))


def sparse_spectral_terms(edge_index, S, w, batch, nb):
    n = S.size(0)
    src, dst = edge_index[0], edge_index[1]
    d = _seg_sum(w, src, n)
    tr = _seg_sum(w * (S[src] * S[dst]).sum(-1), batch[src], nb)
    m2 = 2 * (_seg_sum(w, batch[src], nb) / 2).clamp(min=EPS)
    ca = _seg_sum(S * d.unsqueeze(-1), batch, nb)
    return -(tr - (ca * ca).sum(-1) / m2) / m2, tr.abs() / m2


def unbatched_cluster_terms(S, batch, nb):
    n = torch.bincount(batch, minlength=nb)[:nb].to(S.dtype)
    return _seg_sum(S, batch, nb).norm(dim=-1) / n * math.sqrt(S.size(1)) - 1


def unbatched_ortho_terms(S, batch, nb):
    return torch.stack([ortho_terms(S[batch == g].unsqueeze(0))[0] for g in range(nb)])


def selector(params, dtype):
    """(weights, biases) of MLPSelect's Linear layers from a state dict, as leaves of the given dtype."""
    idx = sorted({int(k.split(".")[3]) for k in params if k.startswith("selector.mlp.lins.")})
    ws = [params[f"selector.mlp.lins.{i}.weight"].to(dtype).clone().requires_grad_(True) for i in idx]
    bs = [params[f"selector.mlp.lins.{i}.bias"].to(dtype).clone().requires_grad_(True) for i in idx]
    names = [f"selector.mlp.lins.{i}.{p}" for i in idx for p in ("weight", "bias")]
    return ws, bs, names


def pool_losses(case, dtype, device="cpu", weights=None, biases=None, x=None):
    """(losses, spectral scale, S, {"x_pool", "adj_pool"}) of a fixture case (``cfg``, ``inputs``, ``params``): the three
    losses with their coefficients, the spectral loss's scale (mean over graphs of |trace(raw)| / 2m), S, and the pooled
    features and (post-processed, oracle) adjacency.  ``weights`` / ``biases`` / ``x``: leaves to differentiate."""
    cfg, inp = case["cfg"], case["inputs"]
    batched = case["alias"] == "dmon"
    if weights is None:
        weights, biases, _ = selector(case["params"], dtype)
    if x is None:
        x = inp["x"].to(dtype)
    x = x.to(device)
    weights = [w.to(device) for w in weights]
    biases = [b.to(device) for b in biases]
    act = cfg.get("act")
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
        raw = s.transpose(1, 2) @ a @ s
        spec, scale = spectral_terms(a, s, raw, mask)
        clu, ort = cluster_terms(s, mask), ortho_terms(s)
        x_pool = s.transpose(1, 2) @ xd
    else:
        s = O.mlp_select(x, weights, biases, None, act)
        bt = batch.to(device) if batch is not None else torch.zeros(x.size(0), dtype=torch.long, device=device)
        nb = int(bt.max()) + 1
        spec, scale = sparse_spectral_terms(ei, s, w, bt, nb)
        clu, ort = unbatched_cluster_terms(s, bt, nb), unbatched_ortho_terms(s, bt, nb)
        raw = torch.zeros(nb, s.size(1), s.size(1), dtype=s.dtype, device=device).index_add_(
            0, bt[ei[0]], w.view(-1, 1, 1) * s[ei[0]].unsqueeze(2) * s[ei[1]].unsqueeze(1))
        x_pool = _seg_sum(s.unsqueeze(2) * x.unsqueeze(1), bt, nb)
    coef = (cfg.get("spectral_loss_coeff", 1.0), cfg.get("cluster_loss_coeff", 1.0), cfg.get("ortho_loss_coeff", 0.0))
    losses = {n: v.mean() * c for n, v, c in zip(LOSSES, (spec, clu, ort), coef)}
    adj_pool = O.postprocess_dense(raw, cfg.get("remove_self_loops", True), cfg.get("degree_norm", True),
                                   cfg.get("adj_transpose", True) if batched else False, cfg.get("edge_weight_norm", False))
    return losses, scale.mean() * coef[0], s, {"x_pool": x_pool, "adj_pool": adj_pool}


def pool_grads(case, dtype, device="cpu"):
    """{loss: (value, {"x": dL/dx, "params": {name: dL/dp}})} of the restatement, each loss differentiated alone."""
    weights, biases, names = selector(case["params"], dtype)
    x = case["inputs"]["x"].to(dtype).clone().requires_grad_(True)
    losses, scale, _, _ = pool_losses(case, dtype, device, weights, biases, x)
    leaves = [x] + [t for pair in zip(weights, biases) for t in pair]
    out = {}
    for n in LOSSES:
        g = torch.autograd.grad(losses[n], leaves, retain_graph=True, allow_unused=True)
        g = [torch.zeros_like(l) if gi is None else gi for gi, l in zip(g, leaves)]
        out[n] = (losses[n].detach(), {"x": g[0], "params": dict(zip(names, g[1:]))})
    return out, scale.detach()
