"""LaPool's selector in plain torch, graph by graph: any device, any float dtype, differentiable in ``x``.

Three functions, the three steps of the native path (csrc/lapool.hip), each in the two layouts the selector takes:

- padded: ``x`` [B,N,F], ``adj`` [B,N,N], ``mask`` [B,N] (None: every row real);
- edge list: ``x`` [n,F], ``edge_index`` [2,E] (+ ``edge_weight``), ``batch`` [n] sorted (None: one graph).

Nothing here is sized N_total x K_total: a graph's rows meet that graph's leaders only.  tests/test_lapool_restatement.py
pins it to the reference's fixtures.
"""
from typing import Optional

import torch
from torch import Tensor


def variation(x: Tensor, adj: Optional[Tensor] = None, mask: Optional[Tensor] = None, *,
              edge_index: Optional[Tensor] = None, edge_weight: Optional[Tensor] = None) -> Tensor:
    """v_i = ||deg_i x_i - sum_j a_ij x_j||_2.  Padded: rows and columns of padded nodes count as zero.  Edge list:
    self-loops are dropped, deg is the sum of what is left, duplicates add."""
    if adj is not None:
        a = adj.to(x.dtype)
        if mask is not None:
            m = mask.to(torch.bool)
            a = a * m.unsqueeze(-1) * m.unsqueeze(-2)
        return (a.sum(-1, keepdim=True) * x - torch.bmm(a, x)).norm(dim=-1)
    row, col = edge_index[0], edge_index[1]
    w = torch.ones(row.numel(), dtype=x.dtype, device=x.device) if edge_weight is None \
        else edge_weight.reshape(-1).to(x.dtype)
    keep = row != col
    row, col, w = row[keep], col[keep], w[keep]
    n = x.size(0)
    deg = torch.zeros(n, dtype=x.dtype, device=x.device).index_add_(0, row, w)
    ax = torch.zeros_like(x).index_add_(0, row, w.unsqueeze(-1) * x[col])
    return (deg.unsqueeze(-1) * x - ax).norm(dim=-1)


def _segments(n: int, batch: Optional[Tensor]):
    if batch is None or batch.numel() == 0:
        return [(0, n)]
    sizes = torch.bincount(batch).tolist()
    out, at = [], 0
    for c in sizes:
        out.append((at, at + c))
        at += c
    return out


def leaders_from(v: Tensor, adj: Optional[Tensor] = None, mask: Optional[Tensor] = None, *,
                 edge_index: Optional[Tensor] = None, batch: Optional[Tensor] = None) -> Tensor:
    """leader_i = real and v_i >= v_j for every neighbour j; a graph with a real node and no leader makes every real
    node a leader.  Padded: neighbours are the nonzero entries on real columns.  Edge list: the entries that are no
    self-loop, explicit zero weights included.  Compares the floats it is given: no tolerance."""
    if adj is not None:
        B, N = v.shape
        m = torch.ones(B, N, dtype=torch.bool, device=v.device) if mask is None else mask.to(torch.bool)
        out = torch.zeros(B, N, dtype=torch.bool, device=v.device)
        for b in range(B):
            nb = (adj[b] != 0) & m[b].unsqueeze(0)
            ge = v[b].unsqueeze(1) >= v[b].unsqueeze(0)
            lead = ~(nb & ~ge).any(dim=1) & m[b]
            if bool(m[b].any()) and not bool(lead.any()):
                lead = m[b].clone()
            out[b] = lead
        return out
    n = v.numel()
    row, col = edge_index[0], edge_index[1]
    keep = row != col
    row, col = row[keep], col[keep]
    lead = torch.ones(n, dtype=torch.bool, device=v.device)
    lead[row[~(v[row] >= v[col])]] = False
    for lo, hi in _segments(n, batch):
        if hi > lo and not bool(lead[lo:hi].any()):
            lead[lo:hi] = True
    return lead


def _assign_graph(x: Tensor, lead: Tensor, eps: float) -> Tensor:
    """One graph's real rows ``x`` [n,F] and leader flags [n] -> [n, k]."""
    xl = x[lead]
    k = xl.size(0)
    z = (x @ xl.t()) / (x.norm(dim=-1, keepdim=True) * xl.norm(dim=-1, keepdim=True).t() + eps)
    s = torch.softmax(z, dim=-1)
    cols = torch.cumsum(lead.to(torch.long), 0) - 1
    hot = torch.nn.functional.one_hot(cols.clamp_min(0), max(k, 1))[:, :k].to(x.dtype)
    return torch.where(lead.unsqueeze(-1), hot, s)


def assign(x: Tensor, leader_mask: Tensor, mask: Optional[Tensor] = None, batch: Optional[Tensor] = None,
           eps: float = 1e-8) -> Tensor:
    """S: per graph softmax_c(x_i . x_l(c) / (|x_i| |x_l(c)| + eps)) over the graph's own leaders in node order, leader
    rows one-hot, padded rows and the columns from k_b on zero.  [B,N,K_max] for ``x`` [B,N,F], [n,K_max] for [n,F]."""
    lm = leader_mask.to(torch.bool)
    if x.dim() == 3:
        B, N, _ = x.shape
        m = torch.ones(B, N, dtype=torch.bool, device=x.device) if mask is None else mask.to(torch.bool)
        lm = lm & m
        kmax = int(lm.sum(1).max()) if B and N else 0
        out = torch.zeros(B, N, kmax, dtype=x.dtype, device=x.device)
        for b in range(B):
            idx = m[b].nonzero(as_tuple=True)[0]
            if idx.numel() == 0:
                continue
            sb = _assign_graph(x[b, idx], lm[b, idx], eps)
            out[b, idx, :sb.size(1)] = sb
        return out
    n = x.size(0)
    segs = _segments(n, batch)
    kmax = max([int(lm[lo:hi].sum()) for lo, hi in segs] + [0])
    out = torch.zeros(n, kmax, dtype=x.dtype, device=x.device)
    for lo, hi in segs:
        if hi > lo:
            sb = _assign_graph(x[lo:hi], lm[lo:hi], eps)
            out[lo:hi, :sb.size(1)] = sb
    return out


def select(x: Tensor, adj: Optional[Tensor] = None, mask: Optional[Tensor] = None, *,
           edge_index: Optional[Tensor] = None, edge_weight: Optional[Tensor] = None,
           batch: Optional[Tensor] = None, eps: float = 1e-8):
    """(v, leader mask, S) of one selector call; the leader set is found without gradient."""
    with torch.no_grad():
        v = variation(x, adj, mask, edge_index=edge_index, edge_weight=edge_weight)
        lead = leaders_from(v, adj, mask, edge_index=edge_index, batch=batch)
    return v, lead, assign(x, lead, mask=mask, batch=batch, eps=eps)


def densify(x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], batch: Optional[Tensor]):
    """(x [B,N,F], adj [B,N,N], mask [B,N]) of a sorted batch: what a batched pooler makes of a sparse input (duplicates
    add, explicit zeros stay zero)."""
    b = batch if batch is not None else torch.zeros(x.size(0), dtype=torch.long, device=x.device)
    sizes = torch.bincount(b)
    ptr = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])
    B, N = sizes.numel(), int(sizes.max())
    adj = torch.zeros(B, N, N, dtype=x.dtype, device=x.device)
    w = torch.ones(edge_index.size(1), dtype=x.dtype, device=x.device) if edge_weight is None \
        else edge_weight.reshape(-1).to(x.dtype)
    g = b[edge_index[0]]
    adj.index_put_((g, edge_index[0] - ptr[g], edge_index[1] - ptr[g]), w, accumulate=True)
    loc = torch.arange(x.size(0), device=x.device) - ptr[b]
    xd = torch.zeros(B, N, x.size(1), dtype=x.dtype, device=x.device)
    xd[b, loc] = x
    mask = torch.zeros(B, N, dtype=torch.bool, device=x.device)
    mask[b, loc] = True
    return xd, adj, mask


def case_select(case: dict, dtype=torch.float32, device="cpu"):
    """(x as the selector sees it, v, leader mask, S) of one stored fixture case, in the layout the case runs in; ``x``
    is a leaf that requires grad."""
    inp = {k: (v.to(device) if isinstance(v, Tensor) else v) for k, v in case["inputs"].items()}
    x = inp["x"].to(dtype)
    ew = inp.get("edge_weight")
    ew = None if ew is None else ew.to(dtype)
    if inp.get("adj") is not None:
        x = x.clone().requires_grad_(True)
        return (x,) + select(x, inp["adj"].to(dtype), inp.get("mask"))
    if case["cfg"].get("batched", True):
        xd, adj, mask = densify(x, inp["edge_index"], ew, inp.get("batch"))
        xd.requires_grad_(True)
        return (xd,) + select(xd, adj, mask)
    x = x.clone().requires_grad_(True)
    return (x,) + select(x, edge_index=inp["edge_index"], edge_weight=ew, batch=inp.get("batch"))
