"""ASAP pooling's fitness, selection and Reduce restated in plain torch (no custom kernels, no reference import), twice:

* :func:`fitness_reference_shaped` -- the operators in the order the reference applies them: gather ``x_pool[src]``,
  scatter-max, the ``F x F`` ``Linear``, ``att`` on the concatenation, leaky ReLU, PyG's edge softmax (``+ 1e-16``),
  the weighted scatter-sum of ``x[src]``, and LEConv as PyG's code computes it,
  ``out_i = lin3(x_i) + sum_{e: dst(e) = i} w_e (lin1(x_src(e)) - lin2(x_i))``.
* :func:`fitness_collapsed` -- the form the kernels use.  ``att`` splits into a query half ``a1`` and a source half
  ``a2``, so with ``w~ = W^T a1`` and ``c = <a1, b_lin> + b_att`` the logit is ``leaky(sq[dst] + sp[src])``,
  ``sq = <x_q, w~> + c``, ``sp = <x_pool, a2>``: the ``Linear`` is never applied to a row.  LEConv at one channel is
  ``p3_i + b3 + sum_e w_e p1[src_e] + (b1 - p2_i) W_i`` with ``p_k = <x_new, w_k>`` and ``W_i`` the summed weight of i's
  in-edges.

Both work on the list that already has its self-loops (:func:`add_remaining_self_loops`: the non-loop edges in their
order, then one loop per node carrying the weight of the node's last loop, or 1), on any device and float dtype.
"""
import torch

import sag_restatement as S

select, assignment = S.select, S.assignment


def add_remaining_self_loops(edge_index, edge_weight, n, fill=1.0):
    keep = edge_index[0] != edge_index[1]
    loop = torch.arange(n, dtype=edge_index.dtype, device=edge_index.device)
    out = torch.cat([edge_index[:, keep], torch.stack([loop, loop])], 1)
    if edge_weight is None:
        return out, None
    lw = torch.full((n,), fill, dtype=edge_weight.dtype, device=edge_weight.device)
    for e in (~keep).nonzero().view(-1).tolist():  # list order: a node's last loop decides
        lw[edge_index[0, e]] = edge_weight[e]
    return out, torch.cat([edge_weight[keep], lw])


def graphconv(x, edge_index, edge_weight, par, prefix="gnn_intra_cluster."):
    msg = x[edge_index[0]] if edge_weight is None else x[edge_index[0]] * edge_weight.view(-1, 1)
    agg = torch.zeros_like(x).index_add(0, edge_index[1], msg)
    return agg @ par[prefix + "lin_rel.weight"].t() + par[prefix + "lin_rel.bias"] + x @ par[prefix + "lin_root.weight"].t()


def scatter_max(rows, dst, n):
    return rows.new_zeros(n, rows.size(1)).scatter_reduce(0, dst.view(-1, 1).expand_as(rows), rows, reduce="amax",
                                                          include_self=False)


def softmax(l, dst, n):
    mx = l.new_zeros(n).scatter_reduce(0, dst, l.detach(), reduce="amax", include_self=False)
    ex = (l - mx[dst]).exp()
    return ex / (l.new_zeros(n).index_add(0, dst, ex) + 1e-16)[dst]


def fitness_reference_shaped(x, x_pool, edge_index, edge_weight, par, negative_slope=0.2, mask=None):
    """(alpha [E'], x_new [N,F], fitness [N])."""
    n, (src, dst) = x.size(0), edge_index
    x_pool_j = x_pool[src]
    x_q = scatter_max(x_pool_j, dst, n) @ par["lin.weight"].t() + par["lin.bias"]
    logit = torch.cat([x_q[dst], x_pool_j], -1) @ par["att.weight"].t() + par["att.bias"]
    alpha = softmax(torch.nn.functional.leaky_relu(logit.view(-1), negative_slope), dst, n)
    if mask is not None:
        alpha = alpha * mask
    x_new = torch.zeros_like(x).index_add(0, dst, x[src] * alpha.view(-1, 1))
    a = x_new @ par["select_scorer.lin1.weight"].t() + par["select_scorer.lin1.bias"]
    b = x_new @ par["select_scorer.lin2.weight"].t()
    msg = a[src] - b[dst]
    if edge_weight is not None:
        msg = msg * edge_weight.view(-1, 1)
    fit = torch.zeros_like(a).index_add(0, dst, msg) + x_new @ par["select_scorer.lin3.weight"].t() \
        + par["select_scorer.lin3.bias"]
    return alpha, x_new, fit.view(-1)


def collapse(par):
    """(w~ [F], c scalar tensor, a2 [F]) of the attention logit."""
    F = par["lin.weight"].size(0)
    a1, a2 = par["att.weight"].view(-1)[:F], par["att.weight"].view(-1)[F:]
    return par["lin.weight"].t() @ a1, a1 @ par["lin.bias"] + par["att.bias"].view(()), a2


def master_query(x_pool, edge_index, n):
    """(max rows [N,F], the edge position that gave each entry [N,F]; ties to the lower position)."""
    src, dst = edge_index
    rows = x_pool[src]
    mx = scatter_max(rows, dst, n)
    pos = torch.arange(src.numel(), device=src.device).view(-1, 1).expand_as(rows)
    big = torch.full_like(pos, src.numel())
    cand = torch.where(rows == mx[dst], pos, big)
    arg = torch.full((n, rows.size(1)), src.numel(), dtype=torch.long, device=src.device).scatter_reduce(
        0, dst.view(-1, 1).expand_as(rows), cand, reduce="amin", include_self=True)
    return mx, arg


def fitness_collapsed(x, x_pool, edge_index, edge_weight, par, negative_slope=0.2, mask=None):
    """(alpha, x_new, fitness) without the F x F Linear and with LEConv as three projections."""
    n, (src, dst) = x.size(0), edge_index
    wt, c, a2 = collapse(par)
    sq = master_query(x_pool, edge_index, n)[0] @ wt + c
    sp = x_pool @ a2
    alpha = softmax(torch.nn.functional.leaky_relu(sq[dst] + sp[src], negative_slope), dst, n)
    if mask is not None:
        alpha = alpha * mask
    x_new = torch.zeros_like(x).index_add(0, dst, x[src] * alpha.view(-1, 1))
    return alpha, x_new, leconv_collapsed(x_new, edge_index, edge_weight, par)


def leconv_collapsed(x_new, edge_index, edge_weight, par, prefix="select_scorer."):
    n, (src, dst) = x_new.size(0), edge_index
    p1, p2, p3 = (x_new @ par[prefix + f"lin{k}.weight"].view(-1) for k in (1, 2, 3))
    w = torch.ones(src.numel(), dtype=x_new.dtype, device=x_new.device) if edge_weight is None else edge_weight
    wsum = torch.zeros_like(p1).index_add(0, dst, w)
    agg = torch.zeros_like(p1).index_add(0, dst, w * p1[src])
    return p3 + par[prefix + "lin3.bias"].view(()) + agg + (par[prefix + "lin1.bias"].view(()) - p2) * wsum


def activate(fit, nonlinearity="sigmoid"):
    return {"sigmoid": torch.sigmoid, "tanh": torch.tanh}.get(nonlinearity, lambda v: v)(fit)


def pool_case(case, dtype=torch.float32, collapsed=True, params=None, x=None, perm=None, mask=None):
    """A stored fixture case -> dict(alpha, x_new, fitness, score, perm, weight, x_pool, edge_index, edge_weight).
    ``params`` / ``x``: leaves that replace the stored ones; ``perm`` overrides the selection."""
    i, cfg = case["inputs"], case["cfg"]
    par = {k: v.to(dtype) for k, v in case["params"].items()} if params is None else params
    x = i["x"].to(dtype) if x is None else x
    x = x.view(-1, 1) if x.dim() == 1 else x
    n = x.size(0)
    ew = None if i["edge_weight"] is None else i["edge_weight"].to(dtype)
    ei, ew = add_remaining_self_loops(i["edge_index"], ew, n)
    x_gnn = graphconv(x, ei, ew, par) if case["gnn"] == "graphconv" else x
    form = fitness_collapsed if collapsed else fitness_reference_shaped
    alpha, x_new, fit = form(x, x_gnn, ei, ew, par, cfg.get("negative_slope", 0.2), mask)
    score = activate(fit, cfg.get("nonlinearity", "sigmoid"))
    batch = i["batch"] if i["batch"] is not None else torch.zeros(n, dtype=torch.long, device=x.device)
    if perm is None:
        perm = select(score, batch, cfg.get("ratio", 0.5))
    weight = score[perm]
    return dict(alpha=alpha, x_new=x_new, fitness=fit, score=score, perm=perm, weight=weight,
                x_pool=x_new[perm] * weight.view(-1, 1), edge_index=ei, edge_weight=ew, batch=batch)
