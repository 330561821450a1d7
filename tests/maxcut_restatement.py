"""MaxCut pooling's score net, cut loss, selection, assignment and Reduce restated in plain torch (no custom kernels, no
reference import).  The score net twice:

* :func:`scores_reference_shaped` -- the operators in the order the reference applies them: the delta-GCN matrix
  ``P = I - delta L_sym`` as an explicit ``N_P + E`` edge list (self-loops dropped, degrees by source, ``deg^-1/2`` with
  ``inf -> 0``, the identity appended), then per layer ``lin``, a gather of the projected rows, the weighting, a
  scatter-add and the bias.
* :func:`scores_collapsed` -- the form the kernels use: with ``z = h W^T``,

      h'_i = act((1 - delta) [i < n_P] z_i + delta dinv_i sum_{r -> i, r != i} w_e dinv_r z_r + b),

  ``n_P = max(edge_index) + 1``: the matrix is never formed.

Both take the stored parameter names (``selector.score_net. ...``) and work on any device and float dtype.
"""
import math

import torch

PRE = "selector.score_net."
ACTS = {"identity": lambda t: t, "none": lambda t: t, "tanh": torch.tanh, "relu": torch.relu}


def net_config(cfg):
    """(mp layers, mlp layers, mp_act, mlp_act, act, delta) of a stored ``cfg`` with the pooler's defaults filled in."""
    return (len(cfg.get("mp_units", [32, 32, 32, 32])), len(cfg.get("mlp_units", [16, 16])), cfg.get("mp_act", "tanh"),
            cfg.get("mlp_act", "relu"), cfg.get("act", "tanh"), cfg.get("delta", 2.0))


def _weights(edge_index, edge_weight, dtype):
    if edge_weight is None:
        return torch.ones(edge_index.size(1), dtype=dtype, device=edge_index.device)
    return edge_weight.to(dtype)


def n_p_of(edge_index):
    return int(edge_index.max()) + 1 if edge_index.numel() else 0


def dinv_of(edge_index, w, n):
    keep = edge_index[0] != edge_index[1]
    deg = torch.zeros(n, dtype=w.dtype, device=w.device).index_add(0, edge_index[0][keep], w[keep])
    dinv = deg.pow(-0.5)
    return torch.where(dinv == float("inf"), torch.zeros_like(dinv), dinv)


def delta_gcn_list(edge_index, edge_weight, delta, dtype):
    """(index [2, E' + n_P], value): P as an edge list ``row -> col`` whose entries a convolution sums by ``col``."""
    w = _weights(edge_index, edge_weight, dtype)
    n = n_p_of(edge_index)
    keep = edge_index[0] != edge_index[1]
    ei, w = edge_index[:, keep], w[keep]
    dinv = dinv_of(ei, w, n)
    loop = torch.arange(n, device=edge_index.device)
    value = torch.cat([delta * (dinv[ei[0]] * w * dinv[ei[1]]), torch.full((n,), 1.0 - delta, dtype=dtype,
                                                                           device=edge_index.device)])
    return torch.cat([ei, torch.stack([loop, loop])], 1), value


def _tail(h, par, n_mlp, mlp_act, act):
    for l in range(n_mlp):
        h = ACTS[mlp_act](h @ par[f"{PRE}mlp.{l}.weight"].t() + par[f"{PRE}mlp.{l}.bias"])
    return ACTS[act](h @ par[PRE + "final_layer.weight"].t() + par[PRE + "final_layer.bias"]).view(-1)


def scores_reference_shaped(par, cfg, x, edge_index, edge_weight):
    n_mp, n_mlp, mp_act, mlp_act, act, delta = net_config(cfg)
    index, value = delta_gcn_list(edge_index, edge_weight, delta, x.dtype)
    h = x @ par[PRE + "initial_layer.weight"].t() + par[PRE + "initial_layer.bias"]
    for l in range(n_mp):
        z = h @ par[f"{PRE}mp_convs.{l}.lin.weight"].t()
        h = ACTS[mp_act](torch.zeros_like(z).index_add(0, index[1], z[index[0]] * value.view(-1, 1))
                         + par[f"{PRE}mp_convs.{l}.bias"])
    return _tail(h, par, n_mlp, mlp_act, act)


def layer_collapsed(z, edge_index, w, dinv, n_p, delta, bias=None, act="identity"):
    """One collapsed layer on projected rows ``z`` [N, C]; ``w`` [E] the edge weights, ``dinv`` [N]."""
    keep = edge_index[0] != edge_index[1]
    src, dst = edge_index[0][keep], edge_index[1][keep]
    agg = torch.zeros_like(z).index_add(0, dst, z[src] * (w[keep] * dinv[src]).view(-1, 1))
    # (a row at or above n_P has no diagonal entry at all: a select, not a product with 0, so a NaN there stays out)
    below = (torch.arange(z.size(0), device=z.device) < n_p).view(-1, 1)
    t = torch.where(below, (1.0 - delta) * z, torch.zeros_like(z)) + delta * dinv.view(-1, 1) * agg
    if bias is not None:
        t = t + bias
    return ACTS[act](t)


def scores_collapsed(par, cfg, x, edge_index, edge_weight):
    n_mp, n_mlp, mp_act, mlp_act, act, delta = net_config(cfg)
    w = _weights(edge_index, edge_weight, x.dtype)
    dinv = dinv_of(edge_index, w, x.size(0))
    n_p = n_p_of(edge_index)
    h = x @ par[PRE + "initial_layer.weight"].t() + par[PRE + "initial_layer.bias"]
    for l in range(n_mp):
        z = h @ par[f"{PRE}mp_convs.{l}.lin.weight"].t()
        h = layer_collapsed(z, edge_index, w, dinv, n_p, delta, par[f"{PRE}mp_convs.{l}.bias"], mp_act)
    return _tail(h, par, n_mlp, mlp_act, act)


def cut_loss(s, edge_index, edge_weight, batch):
    """mean over the graphs of s^T A s / vol on the raw list (self-loops and duplicates count; vol = 0 -> 1)."""
    w = _weights(edge_index, edge_weight, s.dtype)
    b = batch if batch is not None else torch.zeros(s.numel(), dtype=torch.long, device=s.device)
    nb = int(b.max()) + 1
    az = torch.zeros_like(s).index_add(0, edge_index[0], w * s[edge_index[1]])
    cut = torch.zeros(nb, dtype=s.dtype, device=s.device).index_add(0, b, s * az)
    vol = torch.zeros(nb, dtype=s.dtype, device=s.device).index_add(0, b[edge_index[0]], w)
    return (cut / torch.where(vol == 0, torch.ones_like(vol), vol)).mean()


def select(score, batch, ratio=0.5):
    """long [K]: the kept nodes graph by graph in descending score; ``ceil(ratio * n)`` in float32, as PyG takes it."""
    out, s = [], score.detach()
    b = batch if batch is not None else torch.zeros(s.numel(), dtype=torch.long, device=s.device)
    for g in range(int(b.max()) + 1):
        idx = (b == g).nonzero().view(-1)
        n = idx.numel()
        k = min(int(ratio), n) if isinstance(ratio, int) or ratio >= 1 else int(
            math.ceil(float(torch.tensor(float(ratio), dtype=torch.float32) * torch.tensor(float(n), dtype=torch.float32))))
        out.append(idx[torch.sort(s[idx], descending=True, stable=True)[1][:k]])
    return torch.cat(out)


def assign_rounds(kept_sorted, edge_index, n, max_iter):
    """Python lists: label [n] (1 .. K by position in ``kept_sorted``, 0 = none) after up to ``max_iter`` rounds.  A round
    reads the labels of its start; an unlabelled node takes the label most of its labelled sources carry, duplicates
    counted, the lowest label on a tie."""
    label = [0] * n
    for pos, node in enumerate(kept_sorted.tolist()):
        label[node] = pos + 1
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    for _ in range(max_iter):
        votes = {}
        for r, i in zip(src, dst):
            if label[i] == 0 and label[r] > 0:
                votes.setdefault(i, {}).setdefault(label[r], 0)
                votes[i][label[r]] += 1
        if not votes:
            break
        new = list(label)
        for i, v in votes.items():
            top = max(v.values())
            new[i] = min(l for l, c in v.items() if c == top)
        label = new
    return label


def cluster_index_of(kept, edge_index, n, max_iter):
    """long [n]: every node's supernode (the rank of its kept node among the kept nodes in ascending node order), or -1
    where the rounds left the node unassigned."""
    kept_sorted = torch.sort(kept)[0]
    label = torch.tensor(assign_rounds(kept_sorted, edge_index, n, max_iter), dtype=torch.long)
    return label - 1


def reduce(x, scores, kept, cluster_index, assign_all):
    """x_pool of BaseReduce: the score-weighted sum of every supernode's rows (``assign_all``: supernodes in ascending
    order of their kept node), else the kept rows gated by their score (supernodes in the selection's order)."""
    if not assign_all:
        return x[kept] * scores[kept].view(-1, 1)
    k = int(cluster_index.max()) + 1
    return torch.zeros(k, x.size(1), dtype=x.dtype, device=x.device).index_add(0, cluster_index, x * scores.view(-1, 1))


def pool_case(case, dtype=torch.float32, collapsed=False, params=None, x=None, kept=None):
    """(scores, kept nodes, cluster index, x_pool, loss) of a stored fixture case in ``dtype``.  ``kept`` overrides the
    selection (a float64 run that must keep the float32 nodes)."""
    i, cfg = case["inputs"], case["cfg"]
    par = {k: v.to(dtype) for k, v in case["params"].items()} if params is None else params
    x = i["x"].to(dtype) if x is None else x
    ew = None if i["edge_weight"] is None else i["edge_weight"].to(dtype)
    fn = scores_collapsed if collapsed else scores_reference_shaped
    scores = fn(par, cfg, x, i["edge_index"], ew)
    if kept is None:
        kept = select(scores, i["batch"], cfg.get("ratio", 0.5))
    assign_all = cfg.get("assign_all_nodes", True)
    ci = cluster_index_of(kept, i["edge_index"], x.size(0), cfg.get("max_iter", 5)) if assign_all else None
    x_pool = reduce(x, scores, kept, ci, assign_all) if ci is None or int(ci.min()) >= 0 else None
    loss = cut_loss(scores, i["edge_index"], ew, i["batch"]) * cfg.get("loss_coeff", 1.0)
    return {"scores": scores, "kept": kept, "cluster_index": ci, "x_pool": x_pool, "loss": loss}
