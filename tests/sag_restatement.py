"""SAGPooling's score, selection and Reduce restated in plain torch (no custom kernels), in the project-then-aggregate
form the kernels use: the yardstick of the SAG tests and, run on device tensors, nothing more than a handful of ATen ops.

* **Score.**  ``p = x w_rel``, ``q = x w_root``; ``t_i = (sum_{e: dst(e) = i} p[src(e)] [/ max(indeg_i, 1)] + b) + q_i``.
  With one output channel this is ``lin_rel(aggr_j x_j) + lin_root(x_i)`` of PyG's ``GraphConv`` (``aggr="add"``) and
  ``SAGEConv`` (``aggr="mean"``, ``lin_l`` / ``lin_r``): projection and aggregation commute.
* **Activation.**  ``tanh`` or identity in ratio mode; with ``min_score`` the per-graph softmax of PyG's ``softmax``
  (``+ 1e-16`` in the denominator).
* **Selection.**  PyG's ``topk``: per graph the ``ceil(ratio * n)`` (float ratio) or ``min(ratio, n)`` (int ratio) best
  scores in descending order, or every score above ``min(min_score, max of the graph - 1e-7)`` in node order.  The
  kept node at position c is supernode c; the stored assignment lists the kept nodes ascending with their supernodes.
* **Reduce.**  ``x_pool[c] = multiplier * score[kept[c]] * x[kept[c]]``.

Works on any device and float dtype.
"""
import math

import torch

WEIGHTS = {"graphconv": ("gnn.lin_rel.weight", "gnn.lin_root.weight", "gnn.lin_rel.bias"),
           "sage": ("gnn.lin_l.weight", "gnn.lin_r.weight", "gnn.lin_l.bias")}


def project(x, w_rel, w_root):
    return x @ w_rel.reshape(-1).to(x.dtype), x @ w_root.reshape(-1).to(x.dtype)


def aggregate(p, edge_index, n, mean):
    s = torch.zeros(n, dtype=p.dtype, device=p.device).index_add(0, edge_index[1], p[edge_index[0]])
    if mean:
        deg = torch.zeros(n, dtype=p.dtype, device=p.device).index_add(
            0, edge_index[1], torch.ones(edge_index.size(1), dtype=p.dtype, device=p.device))
        s = s / deg.clamp(min=1)
    return s


def raw_score(x, edge_index, w_rel, w_root, bias, mean=False):
    p, q = project(x, w_rel, w_root)
    t = aggregate(p, edge_index, x.size(0), mean)
    if bias is not None:
        t = t + bias.reshape(-1).to(x.dtype)[0]
    return t + q


def segment_softmax(t, batch, nb):
    mx = torch.full((nb,), float("-inf"), dtype=t.dtype, device=t.device).scatter_reduce(
        0, batch, t.detach(), reduce="amax", include_self=True)
    ex = (t - mx[batch]).exp()
    return ex / (torch.zeros(nb, dtype=t.dtype, device=t.device).index_add(0, batch, ex) + 1e-16)[batch]


def activate(t, batch, nonlinearity="tanh", min_score=None):
    if min_score is not None:
        return segment_softmax(t, batch, int(batch.max()) + 1)
    return torch.tanh(t) if nonlinearity == "tanh" else t


def select(score, batch, ratio=0.5, min_score=None):
    """long [K]: the kept nodes in PyG's order -- graph by graph, descending score in ratio mode (ties to the lower node),
    ascending node in ``min_score`` mode; position c is supernode c.  ``ceil(ratio * n)`` is taken in float32, as PyG does."""
    out = []
    s = score.detach()
    for g in range(int(batch.max()) + 1):
        idx = (batch == g).nonzero().view(-1)
        if min_score is not None:
            out.append(idx[s[idx] > min(float(min_score), float(s[idx].max()) - 1e-7)])
            continue
        n = idx.numel()
        k = min(int(ratio), n) if isinstance(ratio, int) or ratio >= 1 else int(
            math.ceil(float(torch.tensor(float(ratio), dtype=torch.float32) * torch.tensor(float(n), dtype=torch.float32))))
        out.append(idx[torch.argsort(s[idx], descending=True, stable=True)[:k]])
    return torch.cat(out)


def assignment(perm):
    """(node_index ascending, cluster_index): the sparse S the selector stores for the kept nodes ``perm``."""
    node_index, order = torch.sort(perm)
    return node_index, order


def pool(x, edge_index, batch, w_rel, w_root, bias, mean=False, nonlinearity="tanh", ratio=0.5, min_score=None,
         multiplier=1.0, attn=None, perm=None):
    """(raw score, activated score, kept nodes in supernode order, their weights, x_pool) in the dtype of ``x``.
    ``perm`` overrides the selection (a float64 run that must keep the float32 nodes)."""
    a = x if attn is None else attn
    a = a.view(-1, 1) if a.dim() == 1 else a
    b = batch if batch is not None else torch.zeros(x.size(0), dtype=torch.long, device=x.device)
    raw = raw_score(a, edge_index, w_rel, w_root, bias, mean)
    score = activate(raw, b, nonlinearity, min_score)
    if perm is None:
        perm = select(score, b, ratio, min_score)
    weight = score[perm]
    x_pool = x[perm] * weight.view(-1, 1)
    return raw, score, perm, weight, x_pool * multiplier if multiplier != 1 else x_pool


def pool_case(case, dtype=torch.float32, params=None, x=None, perm=None):
    """:func:`pool` on a stored fixture case (``params``: leaves that replace the stored ones)."""
    i, cfg = case["inputs"], case["cfg"]
    names = WEIGHTS[case["gnn"]]
    par = {k: v.to(dtype) for k, v in case["params"].items()} if params is None else params
    attn = i.get("attn")
    return pool(i["x"].to(dtype) if x is None else x, i["edge_index"], i["batch"], par[names[0]], par[names[1]],
                par[names[2]], mean=cfg.get("aggr", "mean" if case["gnn"] == "sage" else "add") == "mean",
                nonlinearity=cfg.get("nonlinearity", "tanh"), ratio=cfg.get("ratio", 0.5),
                min_score=cfg.get("min_score"), multiplier=cfg.get("multiplier", 1.0),
                attn=None if attn is None else attn.to(dtype), perm=perm)
