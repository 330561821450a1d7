"""What the family sweep compares against: the plain-torch restatements (tests/*_restatement.py, each pinned to the
reference's fixtures by its own CPU test) called on a draw of tests/fuzz_inputs.py, in float64 or float32 on the CPU.

``reference(draw, dtype)`` -> (float outputs by name, leaves by name): the form ``grad_path_errors`` takes as its oracle.
``exact(draw)`` -> the integer outputs (selections, clusters, counts, tie counts), compared with ``torch.equal``.
Host only."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import acc_restatement as RA  # noqa: E402
import bnpool_restatement as RB  # noqa: E402
import dmon_restatement as RD  # noqa: E402
import edgepool_restatement as RE  # noqa: E402
import hosc_restatement as RH  # noqa: E402
import jb_restatement as RJ  # noqa: E402
import kmis_restatement as RK  # noqa: E402
import lapool_restatement as RL  # noqa: E402
import readout_restatement as RR  # noqa: E402
import sag_restatement as RS  # noqa: E402


def _leaf(t, dtype):
    return None if t is None else t.detach().to(dtype).clone().requires_grad_(True)


# ----------------------------------------------------------------------------------------------------- Just Balance
def jb_finite(d):
    """The graphs whose loss is finite: n_b > 0 (a graph without a real node gives -inf, as the composed form does)."""
    return [b for b, n in enumerate(d["n_b"]) if n > 0]


def jb_rows(d, s, b):
    return s[b] if d["padded"] else s[int(d["ptr"][b]):int(d["ptr"][b + 1])]


def jb_terms(d, s, graphs):
    if not graphs:
        return s.new_zeros(0)
    return torch.stack([RJ.graph_term(jb_rows(d, s, b), d["n_b"][b]) for b in graphs])


def jb_split(d, terms):
    """One output per graph with a real node, from the [B] terms: a graph is never judged through the batch."""
    return {f"term[{b}]": terms[b] for b in jb_finite(d)}


def jb_reference(d, dtype, s=None):
    """"term[b]": the loss of every graph with a real node (the others are checked to be -inf by the caller)."""
    s = _leaf(d["s"], dtype) if s is None else s
    fin = jb_finite(d)
    return dict(zip([f"term[{b}]" for b in fin], jb_terms(d, s, fin).unbind(0))), {"s": s}


def jb_row_mask(d):
    """bool, broadcastable to S: the rows of graphs with a finite loss (the others carry 0 * inf in every form)."""
    fin = torch.zeros(len(d["sizes"]), dtype=torch.bool)
    fin[jb_finite(d)] = True
    return fin.view(-1, 1, 1) if d["padded"] else fin[d["batch"]].view(-1, 1)


# ---------------------------------------------------------------------------------------------------------- BN-Pool
def bnpool_finite(d):
    """The graphs with a real node (the loss of the others divides by n^2 = 0)."""
    return [b for b, n in enumerate(d["n_b"]) if n > 0]


def _bnpool_sub(d, dtype):
    """(graphs with a real node, their S, adj, mask): every graph is on its own, so the others are left out of the
    reference altogether (their 0 / 0 would only put NaN into the shared cluster matrix's gradient)."""
    fin = bnpool_finite(d)
    mask = None if d["mask"] is None else d["mask"][fin]
    return fin, d["s"][fin].to(dtype), d["adj"][fin].to(dtype), mask


def bnpool_operator_reference(d, dtype, t=None):
    """"rec[b]" per graph from the logits T S^T with T and S independent leaves: what the operators compute (their
    backward's P and Q are the gradients to T and to S).  ``t``: the T the operators were given (default S K)."""
    fin, s, adj, mask = _bnpool_sub(d, dtype)
    t = _leaf(s @ d["k_mat"].to(dtype) if t is None else t[fin], dtype)
    s = _leaf(s, dtype)
    n = RB.node_counts(adj, mask)
    rec = RB.rec_terms_from_logits(t @ s.transpose(-1, -2), adj, mask) / (n * n)
    return {f"rec[{b}]": rec[i] for i, b in enumerate(fin)}, {"t": t, "s": s}


def bnpool_reference(d, dtype):
    """"rec[b]" per graph of the public form: leaves S (of the graphs with a real node) and the cluster matrix."""
    fin, s, adj, mask = _bnpool_sub(d, dtype)
    s, k_mat = _leaf(s, dtype), _leaf(d["k_mat"], dtype)
    rec = RB.rec_terms(s, k_mat, adj, mask)
    return {f"rec[{b}]": rec[i] for i, b in enumerate(fin)}, {"s": s, "k_mat": k_mat}


def bnpool_row_mask(d):
    """bool [B,N,1]: the rows inside the mask of graphs with a real node (all others must get exact zeros)."""
    b, n = d["s"].shape[:2]
    m = torch.ones(b, n, dtype=torch.bool) if d["mask"] is None else d["mask"]
    return m.unsqueeze(-1)


# ------------------------------------------------------------------------------------------------------------- DMoN
def dmon_finite(d):
    """The graphs with a real node (the cluster and orthogonality terms of the others are 0 / 0)."""
    return [b for b, n in enumerate(d["n_b"]) if n > 0]


def dmon_reference(d, dtype, raw, grads=False):
    """"spectral[b]", "cluster[b]", "ortho[b]" per graph with a real node; leaves S and ``raw`` = S^T A S as the
    operators were given it (the trace is read from it).  ``grads``: without the orthogonality term where it is constant
    in exact arithmetic (one cluster; one node, whose S^T S / ||S^T S|| is a projector whatever the row): its gradient
    is rounding noise around 0 in any precision."""
    fin = dmon_finite(d)
    s, raw = _leaf(d["s"][fin], dtype), _leaf(raw[fin], dtype)
    mask = d["real"][fin]
    spec, _ = RD.spectral_terms(d["adj"][fin].to(dtype), s, raw, mask)
    terms = {"spectral": spec, "cluster": RD.cluster_terms(s, mask), "ortho": RD.ortho_terms(s)}
    outs = {f"{n}[{b}]": v[i] for n, v in terms.items() for i, b in enumerate(fin)}
    if grads:
        outs = {n: v for n, v in outs.items()
                if not (n.startswith("ortho") and (d["K"] == 1 or d["n_b"][int(n[6:-1])] == 1))}
    return outs, {"s": s, "raw": raw}


def dmon_partial_sums(d, dtype, part_rows, flat=False):
    """(deg [B,N], part [B, nsplit, 2K+2]): row sums of adj on real rows, and per block of ``part_rows`` rows
    (S^T d | S^T 1 | sum d | real rows); ``flat``: as many blocks as the longest un-padded graph needs."""
    s, a, real = d["s"].to(dtype), d["adj"].to(dtype), d["real"].to(dtype)
    deg = a.sum(-1) * real
    b, n, k = s.shape
    nsplit = max(1, -(-(max(d["n_b"]) if flat else n) // part_rows))
    part = torch.zeros(b, nsplit, 2 * k + 2, dtype=dtype)
    for j in range(nsplit):
        lo, hi = j * part_rows, min((j + 1) * part_rows, n)
        sb, db, rb = s[:, lo:hi], deg[:, lo:hi], real[:, lo:hi]
        part[:, j, :k] = torch.einsum("bnk,bn->bk", sb, db)
        part[:, j, k:2 * k] = sb.sum(1)
        part[:, j, 2 * k], part[:, j, 2 * k + 1] = db.sum(1), rb.sum(1)
    return deg, part


def dmon_ds_reference(deg, ca, cs, coef, dtype):
    """out[b,i,k] = coef[b,0] deg[b,i] ca[b,k] + coef[b,1] cs[b,k]."""
    deg, ca, cs, coef = (t.to(dtype) for t in (deg, ca, cs, coef))
    return coef[:, 0].view(-1, 1, 1) * deg.unsqueeze(-1) * ca.unsqueeze(1) + (coef[:, 1:2] * cs).unsqueeze(1)


# ------------------------------------------------------------------------------------------------------------- HOSC
def hosc_reference(d, dtype, raw=None, grads=False):
    """"hosc[b]" = ((1 - alpha) cut + alpha ho_cut) / K and "ortho[b]" = mu x orthogonality per graph with a real node,
    the motif adjacency A A A formed explicitly.  ``raw`` (S^T A S as the operators were given it): a leaf whose trace
    is the first-order cut's numerator.  ``grads``: without the terms that are constant in exact arithmetic (the
    orthogonality of one cluster, MinCut's of one node; the cut of a graph without an edge)."""
    fin = dmon_finite(d)
    s = _leaf(d["s"][fin], dtype)
    adj, mask = d["adj"][fin].to(dtype), d["real"][fin]
    lv = {"s": s}
    den = (adj.sum(-1) * (s * s).sum(-1)).sum(-1)
    if raw is not None and d["alpha"] < 1:
        lv["raw"] = _leaf(raw[fin], dtype)
        cut = -(torch.diagonal(lv["raw"], dim1=-2, dim2=-1).sum(-1) / (den + RH.EPS))
    else:
        cut = RH.cut_terms(adj, s)
    hosc = ((1 - d["alpha"]) * cut + d["alpha"] * RH.ho_cut_terms(adj, s)) / d["K"]
    ortho = RH.hosc_ortho_terms(s, mask.sum(1)) if d["hosc_ortho"] else RH.ortho_terms(s)
    outs = {f"hosc[{b}]": hosc[i] for i, b in enumerate(fin)}
    outs.update({f"ortho[{b}]": d["mu"] * ortho[i] for i, b in enumerate(fin)})
    if grads:
        flat = lambda n: (n.startswith("ortho") and (d["K"] == 1 or (not d["hosc_ortho"] and d["n_b"][int(n[6:-1])] == 1))) \
            or (n.startswith("hosc") and float(d["adj"][int(n[5:-1])].sum()) == 0)  # noqa: E731
        outs = {n: v for n, v in outs.items() if not flat(n)}
    return outs, lv


def hosc_records(d, dtype, z, z1, d3, d1, part_rows, cols=64):
    """part [B, nsplit, K + 4 ceil(K / cols) + 1] of ``hosc_node_terms`` on the padded batch: per block of ``part_rows``
    rows the column square sums of S, then per block of ``cols`` columns (num = sum S (.) Z, den3 = sum d3_i S_ik^2,
    num1 = sum S (.) Z1, den1 = sum d1_i S_ik^2), then the real rows (the layout csrc/hosc.hip documents)."""
    s, real = d["s"].to(dtype), d["real"].to(dtype)
    z, z1, d3, d1 = (t.to(dtype) for t in (z, z1, d3, d1))
    b, n, k = s.shape
    nsplit, nkc = max(1, -(-n // part_rows)), -(-k // cols)
    part = torch.zeros(b, nsplit, k + 4 * nkc + 1, dtype=dtype)
    for j in range(nsplit):
        lo, hi = j * part_rows, min((j + 1) * part_rows, n)
        sb = s[:, lo:hi]
        part[:, j, :k] = (sb * sb).sum(1)
        for c in range(nkc):
            ks = slice(c * cols, min((c + 1) * cols, k))
            sq = (sb[..., ks] ** 2).sum(-1)
            rec = part[:, j, k + 4 * c:k + 4 * c + 4]
            rec[:, 0] = (sb[..., ks] * z[:, lo:hi, ks]).sum((1, 2))
            rec[:, 1] = (d3[:, lo:hi] * sq).sum(1)
            rec[:, 2] = (sb[..., ks] * z1[:, lo:hi, ks]).sum((1, 2))
            rec[:, 3] = (d1[:, lo:hi] * sq).sum(1)
        part[:, j, -1] = real[:, lo:hi].sum(1)
    return part


def hosc_ds_reference(d, dtype, z, zt, z1, z1t, d3, d1, cn, coef):
    """c_num (Z + Zt) + 2 c_den d3 S + c_ortho S / cn + 2 c_den1 d1 S + c_num1 (Z1 + Z1t), coef [B,5] in that order."""
    s = d["s"].to(dtype)
    z, zt, z1, z1t, d3, d1, cn, coef = (t.to(dtype) for t in (z, zt, z1, z1t, d3, d1, cn, coef))
    c = lambda i: coef[:, i].view(-1, 1, 1)  # noqa: E731
    return c(0) * (z + zt) + 2 * c(1) * d3.unsqueeze(-1) * s + c(2) * s / cn.unsqueeze(1) \
        + 2 * c(3) * d1.unsqueeze(-1) * s + c(4) * (z1 + z1t)


def hosc_chain(d, dtype):
    """(d1 = A 1, d3 = A A A 1, z = A A A S) of the padded batch."""
    a, s = d["adj"].to(dtype), d["s"].to(dtype)
    m = a @ a @ a
    return a.sum(-1), m.sum(-1), m @ s


# --------------------------------------------------------------------------------------------------- AsymCheegerCut
def acc_reference(d, dtype):
    """"tv[b]" and "balance[b]" per graph of the padded form (leaf S [B,N,K]); a graph without a node gives 0 and 0."""
    s = _leaf(d["s"], dtype)
    tv, bal = RA.totvar_terms(d["adj"].to(dtype), s), RA.asym_terms(s, d["loss_k"], d["real"])
    outs = {f"tv[{b}]": tv[b] for b in range(len(tv))}
    outs.update({f"balance[{b}]": bal[b] for b in range(len(bal))})
    return outs, {"s": s}


def acc_flat_reference(d, dtype):
    """The same of the un-padded form (leaf S [Ntot,K]): every listed edge counts, duplicates and the hub's included."""
    s = _leaf(d["s_flat"], dtype)
    nb = len(d["n_b"])
    w = None if d["edge_weight"] is None else d["edge_weight"].to(dtype)
    tv = RA.sparse_totvar_terms(d["edge_index"], s, w, d["batch"], nb)
    bal = torch.stack([RA.asym_terms_of(s[int(d["ptr"][b]):int(d["ptr"][b + 1])], d["loss_k"]) for b in range(nb)])
    outs = {f"tv[{b}]": tv[b] for b in range(nb)}
    outs.update({f"balance[{b}]": bal[b] for b in range(nb)})
    return outs, {"s": s}


def acc_colsum(d, dtype, q):
    """[B,K]: sum over a graph's real rows of rho(s_ik - q_k), rho(t) = (k - 1) t for t >= 0 and -t below."""
    out = torch.zeros(q.shape, dtype=dtype)
    for g in range(q.size(0)):
        rows = d["s"][g][d["real"][g]].to(dtype)
        t = rows - q[g].to(dtype)
        out[g] = torch.where(t >= 0, (d["loss_k"] - 1) * t, -t).sum(0)
    return out


def acc_tv_blocks(d, dtype, rows):
    """(part [B, ceil(N / rows)], cnt): per block of ``rows`` rows the sum of a_ij ||s_i - s_j||_1 over the nonzero
    entries of those rows, and their number."""
    a, s = d["adj"].to(dtype), d["s"].to(dtype)
    b, n = a.shape[:2]
    l1 = torch.stack([(g.unsqueeze(1) - g.unsqueeze(0)).abs().sum(-1) for g in s])  # (one graph at a time: [N,N,K])
    per_row, nz = (a * l1).sum(-1), (a != 0).sum(-1)
    nrb = max(1, -(-n // rows))
    pad = nrb * rows - n
    per_row = torch.nn.functional.pad(per_row, (0, pad)).view(b, nrb, rows).sum(-1)
    nz = torch.nn.functional.pad(nz, (0, pad)).view(b, nrb, rows).sum(-1)
    return per_row, nz


def acc_node_tv(d, dtype):
    """[Ntot]: per node the sum over its listed out-edges of w_e ||s_i - s_dst||_1."""
    s, ei = d["s_flat"].to(dtype), d["edge_index"]
    l1 = (s[ei[0]] - s[ei[1]]).abs().sum(-1)
    if d["edge_weight"] is not None:
        l1 = l1 * d["edge_weight"].to(dtype)
    return torch.zeros(s.size(0), dtype=dtype).index_add_(0, ei[0], l1)


def acc_quantile_exact(d, higher=False):
    """q (the float32 entry itself), qnode (the LOWEST row of the graph's real rows that holds it, as a row of the padded
    graph), cge (rows >= q) and nreal, per graph and column; ``higher``: the wrong rule, the highest row."""
    b, n, k = d["s"].shape
    q, node, cge = torch.zeros(b, k), torch.zeros(b, k, dtype=torch.long), torch.zeros(b, k, dtype=torch.long)
    for g in range(b):
        rows_at = d["real"][g].nonzero().view(-1)
        if rows_at.numel() == 0:
            continue
        rows = d["s"][g][rows_at]
        qq, nn = RA.quantile(rows, d["loss_k"])
        if higher:
            nn = rows.size(0) - 1 - (rows.flip(0) == qq).to(torch.int64).argmax(dim=0)
        q[g], node[g], cge[g] = qq, rows_at[nn], (rows >= qq).sum(0)
    return {"q": q, "qnode": node, "cge": cge, "nreal": torch.tensor(d["n_b"])}


# ----------------------------------------------------------------------------------------------------------- LaPool
def lapool_variation(d, dtype):
    x = d["x"].to(dtype)
    if d["padded"]:
        return RL.variation(x, d["adj"].to(dtype), d["mask"])
    w = None if d["edge_weight"] is None else d["edge_weight"].to(dtype)
    return RL.variation(x, edge_index=d["edge_index"], edge_weight=w)


def lapool_leaders(d, v):
    """bool flags for the variations ``v`` as given (float32 values: the comparison has no tolerance)."""
    if d["padded"]:
        return RL.leaders_from(v, d["adj"], d["mask"])
    return RL.leaders_from(v, edge_index=d["edge_index"], batch=d["batch"])


def lapool_columns(d, flags):
    """(col_of: a leader's column inside its graph, -1 otherwise; k [B]) of the leader flags."""
    if d["padded"]:
        f = flags & d["real"]
        col = torch.where(f, torch.cumsum(f.long(), 1) - 1, torch.full_like(f.long(), -1))
        return {"col_of": col.reshape(-1), "k": f.sum(1)}
    col, ks = torch.full((flags.numel(),), -1, dtype=torch.long), []
    for b in range(len(d["n_b"])):
        lo, hi = int(d["ptr"][b]), int(d["ptr"][b + 1])
        f = flags[lo:hi]
        col[lo:hi] = torch.where(f, torch.cumsum(f.long(), 0) - 1, torch.full_like(f.long(), -1))
        ks.append(int(f.sum()))
    return {"col_of": col, "k": torch.tensor(ks)}


def lapool_graph_rows(d, t, b):
    return t[b] if d["padded"] else t[int(d["ptr"][b]):int(d["ptr"][b + 1])]


def lapool_reference(d, dtype, flags):
    """"S[b]" per graph for the leader flags as given; leaf x."""
    x = _leaf(d["x"], dtype)
    s = RL.assign(x, flags, mask=d.get("mask"), batch=d.get("batch"))
    return {f"S[{b}]": lapool_graph_rows(d, s, b) for b in range(len(d["n_b"]))}, {"x": x}


# ---------------------------------------------------------------------------------------------------------- readout
def readout_rows(d, x, w=None):
    rows = x.reshape(-1, x.size(-1))[d["src_rows"]]
    return rows if w is None else rows * w.view(-1, 1)


def readout_reference(d, dtype, ops=None):
    """One output per operation [G, F]; leaves x (and the assignment weights)."""
    x, w = _leaf(d["x"], dtype), _leaf(d.get("weight"), dtype)
    rows = readout_rows(d, x, w)
    outs = {op: RR.scatter(rows, d["index"], d["groups"], op) for op in (d["ops"] if ops is None else ops)}
    return outs, {"x": x, "weight": w}


def readout_exact(d):
    """count [G]; per min / max the number of rows that hold the extreme [G, F] (float32 values, as the kernel sees them)."""
    rows = readout_rows(d, d["x"], d.get("weight"))
    g, idx = d["groups"], d["index"]
    out = {"count": torch.bincount(idx, minlength=g)}
    for op in ("min", "max"):
        if op in d["ops"]:
            ext = RR.scatter(rows, idx, g, op)
            hit = (rows == ext[idx]).to(torch.long)
            out[f"ties_{op}"] = torch.zeros(g, rows.size(1), dtype=torch.long).index_add_(0, idx, hit)
    return out


# -------------------------------------------------------------------------------------------------------------- SAG
def sag_reference(d, dtype):
    x, w_rel, w_root, b = _leaf(d["x"], dtype), _leaf(d["w_rel"], dtype), _leaf(d["w_root"], dtype), _leaf(d["b"], dtype)
    p, q = RS.project(x, w_rel, w_rel if w_root is None else w_root)
    t = RS.aggregate(p, d["edge_index"], d["n"], d["mean"])
    if b is not None:
        t = t + b[0]
    if w_root is not None:
        t = t + q
    return {"p": p, "q": q, "t": t, "a": torch.tanh(t)}, {"x": x, "w_rel": w_rel, "w_root": w_root, "b": b}


def sag_bwd_x_reference(d, dtype, g_q, g_p):
    """dX = g_q (x) w_root + g_p (x) w_rel by autograd through the two projections."""
    x = _leaf(d["x"], dtype)
    w_rel = d["w_rel"].to(dtype)
    w_root = w_rel if d["w_root"] is None else d["w_root"].to(dtype)
    p, q = RS.project(x, w_rel, w_root)
    return torch.autograd.grad([q, p], x, [g_q.to(dtype), g_p.to(dtype)])[0]


# -------------------------------------------------------------------------------------------------------- selectors
def kmis_exact(d, perm=None):
    perm = d["perm"] if perm is None else perm
    mis, cluster = RK.mis_cluster(d["edge_index"], d["order_k"], perm, d["n"])
    return {"k": torch.tensor(int(mis.sum())), "mis": mis.nonzero().view(-1), "cluster": cluster}


def edge_contract_exact(d, perm=None):
    perm = d["perm"] if perm is None else perm
    match = RE.matching(d["edge_index"], d["n"], perm)
    cluster, k = RE.clusters(d["edge_index"], d["n"], match)
    return {"k": torch.tensor(k), "matched": match.to(torch.long), "match": match.nonzero().view(-1), "cluster": cluster}


def tied_order(score, higher=False):
    """The priority order of tied scores: descending, ties to the LOWER index (the rule); ``higher``: the wrong rule."""
    if not higher:
        return torch.argsort(score, descending=True, stable=True)
    n = score.numel()
    rev = torch.argsort(score.flip(0), descending=True, stable=True)
    return (n - 1) - rev
