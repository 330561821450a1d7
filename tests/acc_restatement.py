"""A torch restatement of AsymCheegerCut pooling's two auxiliary losses (reference poolers/asym_cheeger_cut.py,
utils/losses.py:503-550, 780-1010) in this project's own words, for float32 and float64 on any device.

Total variation, per graph:  sum over the edges (i, j) of a_ij ||s_i - s_j||_1 / (2 E), E clamped to >= 1.
    dense form: the edges are the NONZERO entries of the padded adjacency (no mask is read);
    edge form:  every edge of the list counts for the graph of its source, zero-weight ones included.
Balance (asymmetric norm), per graph of n real nodes, K columns and the loss's k:
    q_c = the (idx+1)-th largest entry of column c, idx = min(floor(n / k), n - 1)
    loss = (n (k-1) - sum_ic rho(s_ic - q_c)) / (n (k-1)),  rho(d) = (k-1) d for d >= 0, -d for d < 0;  0 when n (k-1) = 0.
Each form returns per-graph values; the poolers take the batch mean times their coefficient.

Used as the oracle of tests/test_acc_restatement.py (pinned to the reference's fixtures) and tests/test_gpu_acc.py.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import tgp_oracle as O  # noqa: E402
from dmon_restatement import selector  # noqa: E402,F401  (the selector's leaves from a state dict)

LOSSES = ("total_variation_loss", "balance_loss")


def _seg_sum(src, index, size):
    return src.new_zeros((size,) + tuple(src.shape[1:])).index_add_(0, index, src)


def totvar_terms(adj, S):
    """[B]: the dense form, one graph at a time over the nonzero entries of its adjacency."""
    out = []
    for a, s in zip(adj, S):
        i, j = a.nonzero(as_tuple=True)
        l1 = (s[i] - s[j]).abs().sum(-1)
        out.append((a[i, j] * l1).sum() / (2 * max(i.numel(), 1)))
    return torch.stack(out)


def sparse_totvar_terms(edge_index, S, w, batch, nb):
    """[nb]: the edge form; ``w`` None = unit weights."""
    src, dst = edge_index[0], edge_index[1]
    l1 = (S[src] - S[dst]).abs().sum(-1)
    tv = _seg_sum(l1 if w is None else w * l1, batch[src], nb)
    edges = torch.bincount(batch[src], minlength=nb)[:nb].clamp(min=1)
    return tv / (2 * edges)


def quantile(rows, k):
    """(values [K], node index [K]) of the entry at position min(floor(n / k), n - 1) of every column sorted in
    descending order; among equal entries the LOWEST node index (the package's tie rule)."""
    n = rows.size(0)
    idx = min(n // k, n - 1)
    q = rows.sort(dim=0, descending=True)[0][idx]
    node = (rows == q).to(torch.int64).argmax(dim=0)  # (first True)
    return q, node


def asym_terms_of(rows, k):
    n = rows.size(0)
    beta = n * (k - 1)
    if beta == 0:
        return rows.new_zeros(())
    _, node = quantile(rows.detach(), k)
    q = rows.gather(0, node.unsqueeze(0))[0]  # (differentiable: the gradient lands on that node)
    d = rows - q
    return (beta - torch.where(d >= 0, (k - 1) * d, -d).sum()) / beta


def asym_terms(S, k, mask=None):
    """[B]: the padded form; real nodes by ``mask`` (all N without one)."""
    return torch.stack([asym_terms_of(s if mask is None else s[mask[b]], k) for b, s in enumerate(S)])


def unbatched_asym_terms(S, k, batch, nb):
    return torch.stack([asym_terms_of(S[batch == g], k) for g in range(nb)])


class Restated:
    """The four loss forms as this file states them (per-graph values)."""

    totvar = staticmethod(totvar_terms)
    asym = staticmethod(asym_terms)
    sparse_totvar = staticmethod(sparse_totvar_terms)
    unbatched_asym = staticmethod(unbatched_asym_terms)


def pool_losses(case, dtype, device="cpu", weights=None, biases=None, x=None, forms=Restated):
    """(losses, S, {"x_pool", "adj_pool"}) of a fixture case (``cfg``, ``inputs``, ``params``): the two losses with their
    coefficients, S, and the pooled features and (post-processed, oracle) adjacency.  ``weights`` / ``biases`` / ``x``:
    leaves to differentiate.  ``forms``: whose loss forms to run on the restated S (default: this file's)."""
    cfg, inp = case["cfg"], case["inputs"]
    batched = case["alias"] == "acc"
    k = cfg["k"]
    if weights is None:
        weights, biases, _ = selector(case["params"], dtype)
    if x is None:
        x = inp["x"].to(dtype)
    x = x.to(device)
    weights = [w.to(device) for w in weights]
    biases = [b.to(device) for b in biases]
    act = cfg.get("act")
    w = None
    if "adj" in inp:  # already dense
        a = inp["adj"].to(dtype).to(device)
        given = inp.get("mask")
        mask = (torch.ones(x.shape[:2], dtype=torch.bool) if given is None else given).to(device)
        xd = x
    else:
        ei = inp["edge_index"].to(device)
        w = inp.get("edge_weight")
        w = None if w is None else w.to(dtype).to(device)
        batch = inp.get("batch")
    if batched:
        if "adj" not in inp:
            bt = batch if batch is not None else torch.zeros(x.size(0), dtype=torch.long)
            ones = torch.ones(ei.size(1), dtype=dtype, device=device)
            xd, a, mask = O.dense_preprocessing(x.cpu(), ei.cpu(), (ones if w is None else w).cpu(), bt.cpu(),
                                                cfg.get("adj_transpose", True))
            xd, a, mask = xd.to(device), a.to(device), mask.to(device)
            given = mask
        s = O.mlp_select(xd, weights, biases, mask, act)
        tv, bal = forms.totvar(a, s), forms.asym(s, k, given)
        raw = s.transpose(1, 2) @ a @ s
        x_pool = s.transpose(1, 2) @ xd
    else:
        s = O.mlp_select(x, weights, biases, None, act)
        bt = batch.to(device) if batch is not None else torch.zeros(x.size(0), dtype=torch.long, device=device)
        nb = int(bt.max()) + 1
        tv, bal = forms.sparse_totvar(ei, s, w, bt, nb), forms.unbatched_asym(s, k, bt, nb)
        wd = torch.ones(ei.size(1), dtype=dtype, device=device) if w is None else w
        raw = torch.zeros(nb, s.size(1), s.size(1), dtype=s.dtype, device=device).index_add_(
            0, bt[ei[0]], wd.view(-1, 1, 1) * s[ei[0]].unsqueeze(2) * s[ei[1]].unsqueeze(1))
        x_pool = _seg_sum(s.unsqueeze(2) * x.unsqueeze(1), bt, nb)
    coef = (cfg.get("totvar_coeff", 1.0), cfg.get("balance_coeff", 1.0))
    losses = {n: v.mean() * c for n, v, c in zip(LOSSES, (tv, bal), coef)}
    adj_pool = O.postprocess_dense(raw, cfg.get("remove_self_loops", True), cfg.get("degree_norm", True),
                                   cfg.get("adj_transpose", True) if batched else False, cfg.get("edge_weight_norm", False))
    return losses, s, {"x_pool": x_pool, "adj_pool": adj_pool}


def pool_grads(case, dtype, device="cpu", forms=Restated):
    """{loss: (value, {"x": dL/dx, "params": {name: dL/dp}})} of the restatement, each loss differentiated alone."""
    weights, biases, names = selector(case["params"], dtype)
    x = case["inputs"]["x"].to(dtype).clone().requires_grad_(True)
    losses, _, _ = pool_losses(case, dtype, device, weights, biases, x, forms)
    leaves = [x] + [t for pair in zip(weights, biases) for t in pair]
    out = {}
    for n in LOSSES:
        if losses[n].requires_grad:
            g = torch.autograd.grad(losses[n], leaves, retain_graph=True, allow_unused=True)
        else:  # (k = 1: the balance loss is the constant 0)
            g = [None] * len(leaves)
        g = [torch.zeros_like(l) if gi is None else gi for gi, l in zip(g, leaves)]
        out[n] = (losses[n].detach(), {"x": g[0], "params": dict(zip(names, g[1:]))})
    return out
