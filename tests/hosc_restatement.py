"""A torch restatement of HOSC pooling's two auxiliary losses (reference poolers/hosc.py:269-376, utils/losses.py:39-70,
73-127, 218-316, 392-432, 597-641) in this project's own words, for float32 and float64 on any device.

The motif adjacency M = A A A is formed EXPLICITLY here, the way the reference's batched mode does, so that this oracle
shares nothing with the chain A (A (A S)) the kernels and the package's composed forms use.

Batched form, per graph b of a padded batch (A the densified adjacency, A^T when adj_transpose; S masked):
    cut    = -trace(S^T A S) / (sum_i (A 1)_i |S_i|^2 + eps)
    ho_cut = -trace(S^T M S) / (sum_i (M 1)_i |S_i|^2 + eps)
    hosc   = ((1 - alpha) cut + alpha ho_cut) / k
    ortho  = mu || S^T S / ||S^T S|| - I / sqrt(K) ||   or, hosc_ortho,
             mu (sqrt(K) - sum_j ||S_*j|| / sqrt(n)) / (sqrt(K) - 1),  n = mask.sum(),  0 when K <= 1
Unbatched form, per graph g of an edge list: A_g the graph's dense block (rows = sources), n = its node count.  Each
form returns the batch mean.

Used as the oracle of tests/test_hosc_restatement.py (pinned to the reference's fixtures) and tests/test_gpu_hosc.py.
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tgp_oracle as O  # noqa: E402
from dmon_restatement import ortho_terms, selector  # noqa: E402,F401  (MinCut's orthogonality term; the selector's leaves)

EPS = 1e-8
LOSSES = ("hosc_loss", "ortho_loss")


def cut_terms(adj, S):
    """Per-graph -trace(S^T A S) / (trace(S^T diag(A 1) S) + eps) of a stack of dense adjacencies [B,N,N]."""
    num = torch.diagonal(S.transpose(1, 2) @ adj @ S, dim1=-2, dim2=-1).sum(-1)
    den = (adj.sum(-1) * (S * S).sum(-1)).sum(-1)
    return -(num / (den + EPS))


def ho_cut_terms(adj, S):
    return cut_terms(adj @ adj @ adj, S)


def hosc_ortho_terms(S, n):
    """(sqrt(K) - sum_j ||S_*j|| / sqrt(n)) / (sqrt(K) - 1) per graph of S [B,N,K]; n a number or [B]; 0 for K <= 1.
    An integer tensor n (the batched form's mask.sum(1)) has its square root taken in float32, whatever S's dtype: the
    reference does exactly that (utils/losses.py:638)."""
    k = S.size(-1)
    if k <= 1:
        return S.new_zeros(S.size(0))
    sqrt_n = n.sqrt() if isinstance(n, torch.Tensor) else math.sqrt(n)
    return (math.sqrt(k) - S.norm(dim=-2).sum(-1) / sqrt_n) / (math.sqrt(k) - 1)


def dense_blocks(edge_index, w, batch, nb, dtype):
    """([B,Nmax,Nmax] dense blocks with duplicates summed (rows = sources), per-graph node offsets, sizes)."""
    sizes = torch.bincount(batch, minlength=nb)
    ptr = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])
    nmax = int(sizes.max()) if nb else 0
    a = torch.zeros(nb, nmax, nmax, dtype=dtype, device=w.device)
    g = batch[edge_index[0]]
    a.index_put_((g, edge_index[0] - ptr[g], edge_index[1] - ptr[g]), w.to(dtype), accumulate=True)
    return a, ptr, sizes


def pad_rows(S, batch, ptr, nb, nmax):
    out = S.new_zeros(nb, nmax, S.size(1))
    idx = torch.arange(S.size(0), device=S.device) - ptr[batch]
    return out.index_put((batch, idx), S)


def pool_losses(case, dtype, device="cpu", weights=None, biases=None, x=None):
    """(losses, S, {"x_pool", "adj_pool"}) of a fixture case (``cfg``, ``inputs``, ``params``): the two losses with alpha,
    mu and 1 / k applied, S, and the pooled features and (post-processed, oracle) adjacency.  ``weights`` / ``biases`` /
    ``x``: leaves to differentiate."""
    cfg, inp = case["cfg"], case["inputs"]
    batched = case["alias"] == "hosc"
    alpha, mu, hosc_ortho, k = cfg.get("alpha", 0.5), cfg.get("mu", 0.1), cfg.get("hosc_ortho", False), cfg["k"]
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
        cut, ho = cut_terms(a, s), ho_cut_terms(a, s)
        n = mask.sum(1)  # (the pooler always holds a mask: all true for dense inputs given without one)
        ort = hosc_ortho_terms(s, n) if hosc_ortho else ortho_terms(s)
        x_pool = s.transpose(1, 2) @ xd
    else:
        s = O.mlp_select(x, weights, biases, None, act)
        bt = batch.to(device) if batch is not None else torch.zeros(x.size(0), dtype=torch.long, device=device)
        nb = int(bt.max()) + 1
        a, ptr, sizes = dense_blocks(ei, w, bt, nb, dtype)
        sp = pad_rows(s, bt, ptr, nb, a.size(1))
        cut, ho = cut_terms(a, sp), ho_cut_terms(a, sp)
        ort = hosc_ortho_terms(sp, sizes.to(dtype)) if hosc_ortho else torch.stack(
            [ortho_terms(s[bt == g].unsqueeze(0))[0] for g in range(nb)])
        raw = sp.transpose(1, 2) @ a @ sp
        x_pool = sp.transpose(1, 2) @ pad_rows(x, bt, ptr, nb, a.size(1))
    zero = s.new_zeros(())
    hosc = (1 - alpha) * (cut.mean() / k if alpha < 1 else zero) + alpha * (ho.mean() / k if alpha > 0 else zero)
    losses = {"hosc_loss": hosc, "ortho_loss": mu * ort.mean() if mu != 0 else zero}
    adj_pool = O.postprocess_dense(raw, cfg.get("remove_self_loops", True), cfg.get("degree_norm", True),
                                   cfg.get("adj_transpose", True) if batched else False, cfg.get("edge_weight_norm", False))
    return losses, s, {"x_pool": x_pool, "adj_pool": adj_pool}


def pool_grads(case, dtype, device="cpu"):
    """{loss: (value, {"x": dL/dx, "params": {name: dL/dp}})} of the restatement, each loss differentiated alone."""
    weights, biases, names = selector(case["params"], dtype)
    x = case["inputs"]["x"].to(dtype).clone().requires_grad_(True)
    losses, _, _ = pool_losses(case, dtype, device, weights, biases, x)
    leaves = [x] + [t for pair in zip(weights, biases) for t in pair]
    out = {}
    for n in LOSSES:
        if losses[n].requires_grad:
            g = torch.autograd.grad(losses[n], leaves, retain_graph=True, allow_unused=True)
        else:
            g = [None] * len(leaves)
        g = [torch.zeros_like(l) if gi is None else gi for gi, l in zip(g, leaves)]
        out[n] = (losses[n].detach(), {"x": g[0], "params": dict(zip(names, g[1:]))})
    return out
