"""What the family sweep compares against: the plain-torch restatements (tests/*_restatement.py, each pinned to the
reference's fixtures by its own CPU test) called on a draw of tests/fuzz_inputs.py, in float64 or float32 on the CPU.

``reference(draw, dtype)`` -> (float outputs by name, leaves by name): the form ``grad_path_errors`` takes as its oracle.
``exact(draw)`` -> the integer outputs (selections, clusters, counts, tie counts), compared with ``torch.equal``.
For ASAP and MaxCut the operator layer has every kernel's own plain definition on its own float32 inputs, the public
layer the reference-shaped forms of tests/asap_restatement.py and tests/maxcut_restatement.py (not the collapsed
algebra the kernels use), and the exact outputs are the edge-group index, the arg-max table and the labels.
For GTVConv the operator layer is tests/gtv_restatement.py's ``propagate`` on the drawn rows with autograd's gradients
at the activation input, the edge weights and the rows (what the two backward operators return), the public layer its
``layer`` in sparse and in dense mode; ``gtv_backward_by_hand`` restates the backward operators' formulas for the wrong
stand-ins of tests/test_fuzz_inputs.py.
For PAN the MET matrix is stated as the sum of c_n-weighted dense powers of A_t with the series coefficients c as the
leaf (asserted equal to tests/pan_restatement.py's ``met`` in float64), which gives ``pan_met_bwd``'s per-row shares and
their column sums; the public layer is that matrix through the restatement's ``pool`` on the float64 selection.
For EigenPooling the modes are tests/eigenpool_restatement.py's ``cluster_modes`` group by group (entries compared where
the float64 spectrum separates them), Reduce and Lift their sums written out, the public layer ``collapsed``.
Host only."""
import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import acc_restatement as RA  # noqa: E402
import asap_restatement as RAS  # noqa: E402
import bnpool_restatement as RB  # noqa: E402
import dmon_restatement as RD  # noqa: E402
import edgepool_restatement as RE  # noqa: E402
import eigenpool_restatement as REG  # noqa: E402
import gtv_restatement as RG  # noqa: E402
import hosc_restatement as RH  # noqa: E402
import jb_restatement as RJ  # noqa: E402
import kmis_restatement as RK  # noqa: E402
import lapool_restatement as RL  # noqa: E402
import maxcut_restatement as RM  # noqa: E402
import pan_restatement as RP  # noqa: E402
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


# ------------------------------------------------------------------------------------- the shared edge-group index
def edge_group_exact(edge_index, n, by_destination):
    """What ``kernels.sag_edge_group`` must hold, from a stable host argsort of the same list: ``row_ptr`` [n + 1],
    ``perm`` (the edge positions grouped by the row, list order inside a group; None when the list already ascends in
    that row or is empty: offsets only) and the longest group."""
    tgt = edge_index[1 if by_destination else 0]
    counts = torch.bincount(tgt, minlength=n)
    row_ptr = torch.zeros(n + 1, dtype=torch.long)
    row_ptr[1:] = counts.cumsum(0)
    ascending = tgt.numel() == 0 or bool((tgt[1:] >= tgt[:-1]).all())
    return {"row_ptr": row_ptr, "perm": None if ascending else torch.argsort(tgt, stable=True),
            "max_members": int(counts.max()) if n else 0}


def regrouped_order(edge_index, by_destination):
    """long [E]: the same list in the OTHER index form of that direction with every group's edges in the same order -- a
    list that does not ascend in the grouped row is stably sorted by it (offsets only), one that does is interleaved
    (every group's first edge, then every group's second ...: a permutation again)."""
    tgt = edge_index[1 if by_destination else 0]
    if tgt.numel() == 0 or not bool((tgt[1:] >= tgt[:-1]).all()):
        return torch.argsort(tgt, stable=True)
    first = torch.zeros(int(tgt.max()) + 2, dtype=torch.long)
    first[1:] = torch.bincount(tgt).cumsum(0)
    rank = torch.arange(tgt.numel()) - first[tgt]  # an edge's place inside its group
    return torch.argsort(rank * (int(tgt.max()) + 1) + (int(tgt.max()) - tgt), stable=True)


# ------------------------------------------------------------------------------------------------------------- ASAP
def asap_params(d, dtype):
    """(the restatement's parameters, the drawn ones as leaves by name); a bias that is off is a zero no gradient reaches."""
    par, lv = {}, {}
    for k, v in d["params"].items():
        if v is None:
            par[k] = torch.zeros(d["F"] if k == "lin.bias" else 1, dtype=dtype)
        else:
            par[k] = lv[k] = _leaf(v, dtype)
    return par, lv


def _asap_rows(d, dtype):
    x = _leaf(d["x"], dtype)
    return x, (x if d["same_pool"] else _leaf(d["x_pool"], dtype))


def _asap_mask(d, dtype):
    return None if d["alpha_mask"] is None else d["alpha_mask"].to(dtype)


def _asap_weight(d, dtype):
    return None if d["edge_weight"] is None else d["edge_weight"].to(dtype)


def asap_reference(d, dtype):
    """The public layer, reference-shaped (the F x F Linear on every max row, ``att`` on the concatenation, LEConv as
    PyG's code): "alpha" [E] (masked where a mask is drawn), "x_new" [n, F], "score" [n] = act(fitness)."""
    x, x_pool = _asap_rows(d, dtype)
    par, lv = asap_params(d, dtype)
    alpha, x_new, fit = RAS.fitness_reference_shaped(x, x_pool, d["edge_index"], _asap_weight(d, dtype), par,
                                                     d["negative_slope"], _asap_mask(d, dtype))
    # (alpha leaves the product's node without a gradient path: it is handed out for inspection, so it is a value here)
    return {"alpha": alpha.detach(), "x_new": x_new, "score": RAS.activate(fit, d["act"])}, {"x": x, "x_pool": x_pool, **lv}


def asap_operator_inputs(d):
    """float32 inputs of the operators past the first, as the collapsed restatement hands them on in float32: w~ and c,
    sq and sp, the (masked) alpha, LEConv's three weight rows, the projections p [3, n] and the two biases."""
    with torch.no_grad():
        par, _ = asap_params(d, torch.float32)
        ei, n = d["edge_index"], d["n"]
        wt, c, a2 = RAS.collapse(par)
        sq = RAS.master_query(d["x_pool"], ei, n)[0] @ wt + c
        sp = d["x_pool"] @ a2
        val = RAS.softmax(torch.nn.functional.leaky_relu(sq[ei[1]] + sp[ei[0]], d["negative_slope"]), ei[1], n)
        if d["alpha_mask"] is not None:
            val = val * d["alpha_mask"]
        x_new = torch.zeros_like(d["x"]).index_add(0, ei[1], d["x"][ei[0]] * val.view(-1, 1))
        w3 = torch.cat([par[f"select_scorer.lin{k}.weight"] for k in (1, 2, 3)])
        return {"w_tilde": wt, "c": c.reshape(1), "sq": sq, "sp": sp, "val": val, "w3": w3, "p": w3 @ x_new.t(),
                "b1": par["select_scorer.lin1.bias"], "b3": par["select_scorer.lin3.bias"]}


def asap_edge_softmax(logit, dst, n, drop_65th=False):
    """PyG's edge softmax (``+ 1e-16``).  ``drop_65th``: the wrong form in which the 65th edge of a group (lane 0's second
    trip of a 64-lane loop) never reaches the group's sum."""
    mx = logit.new_zeros(n).scatter_reduce(0, dst, logit.detach(), reduce="amax", include_self=False)
    ex = (logit - mx[dst]).exp()
    add = ex
    if drop_65th and dst.numel():
        order = torch.argsort(dst, stable=True)
        first = torch.zeros(n + 1, dtype=torch.long)
        first[1:] = torch.bincount(dst, minlength=n).cumsum(0)
        lost = order[(torch.arange(dst.numel()) - first[dst[order]]) == 64]
        add = ex.clone()
        add[lost] = 0
    return ex / (logit.new_zeros(n).index_add(0, dst, add) + 1e-16)[dst]


def asap_operator_reference(d, dtype, inp=None, drop_65th=False):
    """Every operator's own plain definition on ITS inputs (``inp``, float32, default :func:`asap_operator_inputs`):
    "sq" = <scatter-max of x_pool[src], w~> + c, "alpha" = the segment softmax of leaky(sq_in[dst] + sp_in[src]),
    "out" = the weighted row sum of x[src] with "proj" = its three projections, "t" / "a" = LEConv's scalar form on p and
    its activation.  Leaves x, x_pool, sq_in, sp_in, logit (per edge, an intermediate), val and p: the backward operators
    are the gradients of sq, alpha and out to them."""
    inp = asap_operator_inputs(d) if inp is None else inp
    (src, dst), n = d["edge_index"], d["n"]
    x, x_pool = _asap_rows(d, dtype)
    lv = {"x": x, "x_pool": x_pool}
    outs = {"sq": RAS.scatter_max(x_pool[src], dst, n) @ inp["w_tilde"].to(dtype) + inp["c"].to(dtype)}
    sq_in, sp_in = _leaf(inp["sq"], dtype), _leaf(inp["sp"], dtype)
    logit = sq_in[dst] + sp_in[src]
    outs["alpha"] = asap_edge_softmax(torch.nn.functional.leaky_relu(logit, d["negative_slope"]), dst, n, drop_65th)
    val = _leaf(inp["val"], dtype)
    outs["out"] = torch.zeros_like(x).index_add(0, dst, x[src] * val.view(-1, 1))
    outs["proj"] = inp["w3"].to(dtype) @ outs["out"].t()
    p = _leaf(inp["p"], dtype)
    w = torch.ones(src.numel(), dtype=dtype) if d["edge_weight"] is None else d["edge_weight"].to(dtype)
    agg = torch.zeros(n, dtype=dtype).index_add(0, dst, w * p[0][src])
    wsum = torch.zeros(n, dtype=dtype).index_add(0, dst, w)
    outs["t"] = p[2] + inp["b3"].to(dtype) + agg + (inp["b1"].to(dtype) - p[1]) * wsum
    outs["a"] = RAS.activate(outs["t"], d["act"])
    lv.update(sq_in=sq_in, sp_in=sp_in, logit=logit, val=val if val.numel() else None, p=p)  # (no leaf without entries)
    return outs, lv


def asap_argmax_exact(d, x_pool=None, higher=False):
    """"max" [n, F] (an entry of the float32 input; 0 for a node without in-edge) and "argpos" [n, F]: the LOWEST edge
    position among the equal maxima of (node, column), -1 for an empty group.  ``higher``: the wrong rule."""
    x_pool = d["x_pool"] if x_pool is None else x_pool
    ei, n = d["edge_index"], d["n"]
    E = ei.size(1)
    mx, arg = RAS.master_query(x_pool, ei, n)
    if higher and E:
        flipped, pos = ei.flip(1), torch.arange(E - 1, -1, -1)  # the last position first: the lowest becomes the highest
        arg_f = RAS.master_query(x_pool, flipped, n)[1]
        arg = torch.where(arg_f < E, pos[arg_f.clamp(max=E - 1)], arg_f)
    return {"max": mx, "argpos": torch.where(arg < E, arg, torch.full_like(arg, -1))}


def asap_tied_sources(d):
    """How many (node, column) maxima are held by two DIFFERENT source rows of the group (duplicates of one row aside)."""
    ei, n = d["edge_index"], d["n"]
    if ei.size(1) == 0:
        return 0
    uniq = torch.unique(ei, dim=1)
    rows = d["x_pool"][uniq[0]]
    hit = (rows == RAS.scatter_max(rows, uniq[1], n)[uniq[1]]).to(torch.long)
    return int((torch.zeros(n, rows.size(1), dtype=torch.long).index_add(0, uniq[1], hit) > 1).sum())


def asap_query_half_matters(d, nodes, loops=True):
    """Does x_new of ``nodes`` depend on ``lin``, its bias and ``att``'s bias at all?  They reach a node only through its
    sq_i, one shift of all of its group's logits, which the group's softmax does not see unless leaky ReLU treats its
    members differently: some group of ``nodes`` must hold logits on both sides of 0 (decided in float64).  Where none
    does, the gradient to those parameters is zero in exact arithmetic and rounding noise in any precision.
    ``loops``: on the list with its remaining self-loops, as the pooler sees it."""
    ei, n = d["edge_index"], d["n"]
    if loops:
        ei, _ = RAS.add_remaining_self_loops(ei, None, n)
    with torch.no_grad():
        wt, c, a2 = RAS.collapse(asap_params(d, torch.float64)[0])
        rows = d["x_pool"].double()
        t = (RAS.master_query(rows, ei, n)[0] @ wt + c)[ei[1]] + (rows @ a2)[ei[0]]
    lo = torch.full((n,), float("inf"), dtype=torch.float64).scatter_reduce(0, ei[1], t, reduce="amin")
    hi = torch.full((n,), float("-inf"), dtype=torch.float64).scatter_reduce(0, ei[1], t, reduce="amax")
    return bool(((lo < 0) & (hi > 0))[nodes].any())


def asap_pool_case(d):
    """The draw as a fixture case of ``asap_restatement.pool_case`` (the whole pooler; the drawn biases all on)."""
    return {"inputs": {"x": d["x"], "edge_index": d["edge_index"], "edge_weight": d["edge_weight"], "batch": d["batch"]},
            "cfg": {"in_channels": d["F"], "ratio": 0.5, "negative_slope": d["negative_slope"], "nonlinearity": d["act"]},
            "params": d["params"], "gnn": None}


# ----------------------------------------------------------------------------------------------------------- MaxCut
def maxcut_operator_inputs(d):
    """float32 inputs of the operators past the first: the rows z [n, C_l] every drawn layer projects from, the rows the
    tail reads, dinv as the float32 restatement gives it."""
    g = torch.Generator().manual_seed(7_000_003 + d["seed"])
    n = d["n"]
    z = [torch.randn(n, c, generator=g) for c in d["widths"]]
    w = RM._weights(d["edge_index"], d["edge_weight"], torch.float32)
    return {"z": z, "h_tail": torch.randn(n, d["widths"][-1], generator=g), "dinv": RM.dinv_of(d["edge_index"], w, n)}


def maxcut_operator_reference(d, dtype, inp=None, n_p=None):
    """Every operator's own plain definition: "dinv", "coef" = w dinv[src], "coef_t" = w dinv[dst]; per drawn layer l
    "h{l}" = ``layer_collapsed`` on z_l with its bias and ``mp_act``, "z_next{l}" = h_l W_{l+1}^T, "lin{l}" the same layer
    without bias and activation (its gradient to z_l is the backward's use of the kernel over the by-source group);
    "tail" = ``_tail`` where the tail fits; "az", "cut", "wsum" by source and "at" = A^T s by destination on the raw list.
    ``n_p``: another diagonal limit than the list's (a wrong stand-in)."""
    inp = maxcut_operator_inputs(d) if inp is None else inp
    ei, n = d["edge_index"], d["n"]
    n_p = d["n_p"] if n_p is None else n_p
    w = RM._weights(ei, d["edge_weight"], dtype)
    dinv = RM.dinv_of(ei, w, n)
    outs = {"dinv": dinv, "coef": w * dinv[ei[0]], "coef_t": w * dinv[ei[1]]}
    par = {k: v.to(dtype) for k, v in d["params"].items()}
    dinv_in, lv = inp["dinv"].to(dtype), {}
    for l in range(len(d["widths"])):
        z = lv[f"z{l}"] = _leaf(inp["z"][l], dtype)
        h = RM.layer_collapsed(z, ei, w, dinv_in, n_p, d["delta"], par[f"{RM.PRE}mp_convs.{l}.bias"], d["mp_act"])
        outs[f"h{l}"] = h
        if l + 1 < len(d["widths"]):
            outs[f"z_next{l}"] = h @ par[f"{RM.PRE}mp_convs.{l + 1}.lin.weight"].t()
        outs[f"lin{l}"] = RM.layer_collapsed(z, ei, w, dinv_in, n_p, d["delta"])
    if d["tail"] != "unfit":
        lv["h_tail"] = _leaf(inp["h_tail"], dtype)
        outs["tail"] = RM._tail(lv["h_tail"], par, len(d["mlp_units"]), d["mlp_act"], d["act"])
    s = lv["s"] = _leaf(d["s"], dtype)
    outs["az"] = torch.zeros(n, dtype=dtype).index_add(0, ei[0], w * s[ei[1]])
    outs["cut"] = s * outs["az"]
    outs["wsum"] = torch.zeros(n, dtype=dtype).index_add(0, ei[0], w)
    outs["at"] = torch.zeros(n, dtype=dtype).index_add(0, ei[1], w * s[ei[0]])
    return outs, lv


def maxcut_reference(d, dtype):
    """The public layer, reference-shaped: "score" [n] of the net on the explicit delta-GCN matrix (leaves x and every
    parameter) and "loss", the cut loss of the drawn scores s (leaf s)."""
    x, s = _leaf(d["x"], dtype), _leaf(d["s"], dtype)
    par = {k: _leaf(v, dtype) for k, v in d["params"].items()}
    ew = None if d["edge_weight"] is None else d["edge_weight"].to(dtype)
    score = RM.scores_reference_shaped(par, d["cfg"], x, d["edge_index"], ew)
    return {"score": score, "loss": RM.cut_loss(s, d["edge_index"], ew, d["batch"])}, {"x": x, "s": s, **par}


def maxcut_labels_exact(d):
    """int64 [n]: the labels (1 .. K by position among the kept nodes, 0 = none) after ``max_iter`` rounds."""
    return torch.tensor(RM.assign_rounds(d["kept"], d["edge_index"], d["n"], d["max_iter"]), dtype=torch.long)


# ---------------------------------------------------------------------------------------------------------- GTVConv
def upstream(case, *shape):
    """The upstream gradient of ``case``: float32 values seeded from the name (what tests/test_gpu_fuzz_families.py
    hands the backward operators)."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(zlib.crc32(case.encode())))


def gtv_skipped(d):
    """bool [E]: the edges the kernels skip (self-loops; every endpoint of a draw is in range)."""
    return d["edge_index"][0] == d["edge_index"][1]


def gtv_operator_reference(d, dtype, case=None):
    """``gtv_restatement.propagate`` on the draw's rows ``h``: "out", the distances "d" [E] (0 at a skipped edge), and the
    gradients of <out, upstream(case + "g")> by autograd -- "g" at the activation's input before the mask (the bias is
    handed in as one leaf row per node, whose gradient that is), "gw" at the edge weights (ones for a list without) and
    "dh" at h.  Leaves "h" and "edge_weight"."""
    case = f"gtv-op-{d['seed']}" if case is None else case
    ei, (n, C) = d["edge_index"], d["h"].shape
    E = ei.size(1)
    h = _leaf(d["h"], dtype)
    w = _leaf(torch.ones(E) if d["edge_weight"] is None else d["edge_weight"], dtype)
    rows = _leaf((torch.zeros(C) if d["bias"] is None else d["bias"]).expand(n, C), dtype)
    with torch.enable_grad():  # (the backward operators' outputs are gradients: also under a caller's no_grad)
        out = RG.propagate(h, ei, w, rows, d["mask"], d["delta"], d["eps"], RG.ACTS[d["act"]])
        dist = torch.zeros(E, dtype=dtype).index_put((gtv_skipped(d).logical_not().nonzero().view(-1),),
                                                     RG.distances(h, ei)[1])
        grads = torch.autograd.grad(out, [rows, w, h], upstream(case + "g", n, C).to(dtype), retain_graph=True,
                                    allow_unused=True)
    g, gw, dh = (torch.zeros_like(t) if v is None else v for t, v in zip((rows, w, h), grads))
    return {"out": out, "d": dist, "g": g, "gw": gw, "dh": dh}, {"h": h, "edge_weight": w}


def gtv_reference(d, dtype):
    """The public layer in sparse mode: ``gtv_restatement.layer`` on x, weight, bias and the list (no mask, as in the
    reference); every parameter and input a leaf."""
    lv = {"x": _leaf(d["x"], dtype), "weight": _leaf(d["weight"], dtype), "bias": _leaf(d["bias"], dtype),
          "edge_weight": _leaf(d["edge_weight"], dtype)}
    out = RG.layer(lv["x"], lv["weight"], lv["bias"], d["edge_index"], lv["edge_weight"], None, d["delta"], d["eps"], d["act"])
    return {"out": out}, lv


def gtv_dense_batch(d):
    """The draw's batch in dense mode: (x [B, N, 5] zero-padded, adj [B, N, N] float32 with duplicate edges added up and
    the loops on its diagonal, mask [B, N] of the real rows)."""
    sizes, ptr, ei = d["sizes"], d["ptr"], d["edge_index"]
    B, N = len(sizes), max(sizes)
    w = torch.ones(ei.size(1)) if d["edge_weight"] is None else d["edge_weight"]
    b = d["batch"][ei[0]]
    adj = torch.zeros(B, N, N).index_put((b, ei[0] - ptr[b], ei[1] - ptr[b]), w, accumulate=True)
    x = torch.zeros(B, N, d["x"].size(1))
    for i, c in enumerate(sizes):
        x[i, :c] = d["x"][int(ptr[i]):int(ptr[i + 1])]
    return x, adj, torch.arange(N).view(1, -1) < torch.tensor(sizes).view(-1, 1)


def gtv_dense_reference(d, dtype):
    """The public layer in dense mode on ``gtv_dense_batch``: "out" [B, N, C]; leaves x, weight, bias."""
    x, adj, mask = gtv_dense_batch(d)
    lv = {"x": _leaf(x, dtype), "weight": _leaf(d["weight"], dtype), "bias": _leaf(d["bias"], dtype)}
    out = RG.layer(lv["x"], lv["weight"], lv["bias"], adj.to(dtype), None, mask, d["delta"], d["eps"], d["act"])
    return {"out": out}, lv


def gtv_in_edge_rank(d):
    """int64 [E]: an edge's place among the in-edges of its destination, in the order of the by-destination index (list
    order inside a node, skipped edges counted: the kernel walks them too)."""
    dst = d["edge_index"][1]
    order = torch.argsort(dst, stable=True)
    first = torch.zeros(d["n"] + 1, dtype=torch.long)
    first[1:] = torch.bincount(dst, minlength=d["n"]).cumsum(0)
    rank = torch.empty_like(dst)
    rank[order] = torch.arange(dst.numel()) - first[dst[order]]
    return rank


def gtv_backward_by_hand(d, dtype, case=None, drop_in_edge=None, slope_from_next_row=False):
    """"g" and "dh" of the operator layer from the kernels' own formulas, without autograd (csrc/gtvconv.hip):
    g = upstream act'(out) mask, s_e = delta <g_i, h_col - h_i>, t_e = -s_e gamma_e / d_e where d_e >= eps, and
    dh_i = g_i (1 - delta sum_out gamma_e) + sum_out t_e sign(h_i - h_col) + sum_in (delta gamma_e g_row - t_e sign(h_row -
    h_i)).  Two wrong stand-ins: ``drop_in_edge`` = k leaves the k-th in-edge (from 1) of every node out of the last sum;
    ``slope_from_next_row`` takes act' from row i + 1."""
    case = f"gtv-op-{d['seed']}" if case is None else case
    ei, (n, C) = d["edge_index"], d["h"].shape
    h = d["h"].to(dtype)
    w = (torch.ones(ei.size(1)) if d["edge_weight"] is None else d["edge_weight"]).to(dtype)
    bias = None if d["bias"] is None else d["bias"].to(dtype)
    out = RG.propagate(h, ei, w, bias, d["mask"], d["delta"], d["eps"], RG.ACTS[d["act"]])
    slope = {"identity": torch.ones_like(out), "relu": (out > 0).to(dtype),
             "elu": torch.where(out > 0, torch.ones_like(out), out + 1)}[d["act"]]
    if slope_from_next_row:
        slope = slope.roll(-1, 0)
    g = upstream(case + "g", n, C).to(dtype) * slope
    if d["mask"] is not None:
        g = g * d["mask"].view(-1, 1).to(dtype)
    keep = gtv_skipped(d).logical_not()
    row, col, wk = ei[0, keep], ei[1, keep], w[keep]
    diff = h[col] - h[row]
    dist = diff.abs().sum(-1)
    gamma = wk / dist.clamp(min=d["eps"])
    s = d["delta"] * (g[row] * diff).sum(-1)
    t = torch.where(dist >= d["eps"], -s * gamma / dist.clamp(min=1e-300), torch.zeros_like(s))
    sign = torch.sign(-diff)  # sign(h_row - h_col)
    inward = d["delta"] * gamma.view(-1, 1) * g[row] - t.view(-1, 1) * sign
    if drop_in_edge is not None:
        inward = inward * (gtv_in_edge_rank(d)[keep] != drop_in_edge - 1).view(-1, 1).to(dtype)
    dh = g * (1 - d["delta"] * torch.zeros(n, dtype=dtype).index_add(0, row, gamma)).view(-1, 1) \
        + torch.zeros_like(h).index_add(0, row, t.view(-1, 1) * sign) + torch.zeros_like(h).index_add(0, col, inward)
    return {"g": g, "dh": dh, "t": torch.zeros(ei.size(1), dtype=dtype).index_put((keep.nonzero().view(-1),), t)}


# -------------------------------------------------------------------------------------------------------------- PAN
_PAN_POWERS = {}


def pan_powers(d, dtype):
    """Per graph of the draw (first node, the dense powers [A_t^0 .. A_t^L], the stored pattern, D^-1/2 of the counted
    degrees) in ``dtype``: constants of the list, kept for the last few draws (the oracle is called once per path)."""
    key = (d["seed"], d["n"], d["edge_index"].size(1), int(d["edge_index"].sum()), dtype)
    if key not in _PAN_POWERS:
        if len(_PAN_POWERS) >= 6:
            _PAN_POWERS.clear()
        ei, L, out = d["edge_index"], d["filter_size"], []
        owner = d["batch"][ei[0]]
        for b, size in enumerate(d["all_sizes"]):
            lo = int(d["ptr"][b])
            local = ei[:, owner == b] - lo
            a = RP.transposed_adjacency(local, size, dtype)
            powers = [torch.eye(size, dtype=dtype)]
            for _ in range(L):
                powers.append(powers[-1] @ a)
            _, pattern, _, deg = RP.met_dense_one(local, torch.ones(L + 1, dtype=dtype), size)
            dinv = deg.pow(-0.5)
            out.append((lo, powers, pattern, torch.where(torch.isinf(dinv), torch.zeros_like(dinv), dinv)))
        _PAN_POWERS[key] = out
    return _PAN_POWERS[key]


def pan_met_from_coefficients(d, dtype, c):
    """(index [2, nnz] row-major, values [nnz]) of M = D^-1/2 (sum_n c_n A_t^n) D^-1/2 on the structural pattern, with the
    series coefficients ``c`` [L + 1] (c_n = w_0 ... w_n) as the differentiable input."""
    idx, val = [], []
    for lo, powers, pattern, dinv in pan_powers(d, dtype):
        s = sum(c[k] * p for k, p in enumerate(powers))
        m = (dinv.view(1, -1) * s) * dinv.view(-1, 1)
        at = pattern.nonzero().t()
        idx.append(at + lo)
        val.append(m[at[0], at[1]])
    return torch.cat(idx, 1), torch.cat(val)


def pan_part_reference(d, dtype, g_values, row_limit=None):
    """part [n, L + 1]: part[i, k] = dinv_i sum_j g_ij dinv_j (A_t^k)_ij over the stored entries of row i -- the share of
    row i in dL/dc_k.  ``row_limit``: a wrong stand-in that stops after that many stored entries of a row."""
    rows, at = [], 0
    for lo, powers, pattern, dinv in pan_powers(d, dtype):
        pos = pattern.nonzero().t()
        gm = torch.zeros(pattern.shape, dtype=dtype).index_put((pos[0], pos[1]), g_values[at:at + pos.size(1)].to(dtype))
        if row_limit is not None:
            gm = gm * (pattern.cumsum(1) <= row_limit).to(dtype)
        at += pos.size(1)
        rows.append(torch.stack([dinv * ((gm * dinv.view(1, -1)) * p).sum(1) for p in powers], 1))
    return torch.cat(rows)


def pan_operator_reference(d, dtype, case=None, row_limit=None):
    """"values" of the MET matrix (from the coefficient form, which equals ``pan_restatement.met`` in float64 to 1e-12:
    asserted), "part" of ``pan_met_bwd`` on upstream(case + "g") and "dc", autograd's gradient at the coefficients
    (part's column sums); the scorer's "score", "dot" and "colsum" on its own drawn inputs.  Leaf "c"."""
    case = f"pan-op-{d['seed']}" if case is None else case
    w = d["weight"].to(dtype)
    c = _leaf(torch.cumprod(w, 0), dtype)
    with torch.enable_grad():
        index, values = pan_met_from_coefficients(d, dtype, c)
        g = upstream(case + "g", values.numel()).to(dtype)
        (dc,) = torch.autograd.grad(values, [c], g, retain_graph=True)
    if dtype == torch.float64:
        idx, val = RP.met(d["edge_index"], w, d["n"], d["batch"])
        assert torch.equal(idx, index) and float((val - values.detach()).abs().max()) <= 1e-12
    x, p, beta = d["score_x"].to(dtype), d["score_p"].to(dtype), d["beta"].to(dtype)
    dot = x @ p
    colsum = torch.zeros(d["n"], dtype=dtype).index_add(0, d["score_index"][1], d["score_values"].to(dtype))
    t = beta[0] * dot + beta[1] * colsum
    return {"values": values, "part": pan_part_reference(d, dtype, g, row_limit), "dc": dc,
            "score": torch.tanh(t) if d["use_tanh"] else t, "dot": dot, "colsum": colsum}, {"c": c}


PAN_EPS = 1e-8  # reference tgp/__init__.py: the sparse Connect drops pooled entries with |value| <= eps


def pan_exact(d):
    """The integer outputs: M's "index" and "row_ptr", the "kept" nodes (ascending; the float64 selection, whose cut the
    draw keeps clear of rounding) and the pooled matrix's "pooled_index".  ``pan_restatement.pool`` keeps every entry of
    the induced submatrix; the reference's sparse Connect then drops those with |value| <= eps (a zero series weight
    leaves exact zeros on the entries only longer walks reach): "pooled_stored" marks the survivors among
    "pooled_all", the float64 values of the whole submatrix."""
    with torch.no_grad():
        index, values = pan_met_from_coefficients(d, torch.float64, torch.cumprod(d["weight"].double(), 0))
        x = d["x"].double()
        h = torch.zeros_like(x).index_add(0, index[0], values.view(-1, 1) * x[index[1]]) @ d["lin_w"].double().t() \
            + d["lin_b"].double()
        _, _, perm, _, _, _, _ = RP.pool(h, index, values, d["batch"], d["p"].double(), d["beta"].double())
        kept = perm.sort().values
        pooled = RP.pool(h, index, values, d["batch"], d["p"].double(), d["beta"].double(), perm=kept)
    row_ptr = torch.zeros(d["n"] + 1, dtype=torch.long)
    row_ptr[1:] = torch.bincount(index[0], minlength=d["n"]).cumsum(0)
    stored = pooled[6].abs() > PAN_EPS
    return {"index": index, "row_ptr": row_ptr, "kept": kept, "pooled_index": pooled[5][:, stored],
            "pooled_stored": stored, "pooled_all": pooled[6]}


def pan_reference(d, dtype, ex=None):
    """PANConv -> PANPooling: "conv_out", "met_values", and on the kept nodes in ascending order (``ex``: ``pan_exact``
    of the draw, the float64 selection) their "weight", "x_pool" and the "pooled_values" of the induced submatrix's
    stored entries.  Every parameter a leaf."""
    ex = pan_exact(d) if ex is None else ex
    kept = ex["kept"]
    lv = {"x": _leaf(d["x"], dtype), "weight": _leaf(d["weight"], dtype), "lin.weight": _leaf(d["lin_w"], dtype),
          "lin.bias": _leaf(d["lin_b"], dtype), "p": _leaf(d["p"], dtype), "beta": _leaf(d["beta"], dtype)}
    index, values = pan_met_from_coefficients(d, dtype, torch.cumprod(lv["weight"], 0))
    h = torch.zeros_like(lv["x"]).index_add(0, index[0], values.view(-1, 1) * lv["x"][index[1]]) @ lv["lin.weight"].t() \
        + lv["lin.bias"]
    _, _, _, weight, x_pool, _, pooled = RP.pool(h, index, values, d["batch"], lv["p"], lv["beta"], perm=kept)
    return {"conv_out": h, "met_values": values, "weight": weight, "x_pool": x_pool,
            "pooled_values": pooled[ex["pooled_stored"]]}, lv


# ------------------------------------------------------------------------------------------------------- EigenPooling
def eigenpool_groups(d):
    """[(group id, its nodes ascending)] of the non-empty (graph, cluster) groups of the modes draw."""
    return [(g, (d["gid"] == g).nonzero().view(-1)) for g in d["gid"].unique().tolist()]


def eigenpool_group_modes(d, dtype):
    """{group id: (modes [m, H], ascending eigenvalues or None)}: ``eigenpool_restatement.cluster_modes`` on the group's
    induced adjacency (``dense_adjacency`` of the whole list) in ``dtype``."""
    a = REG.dense_adjacency(d["edge_index"], d["edge_weight"], 0, d["n"], dtype)
    return {g: REG.cluster_modes(a[nodes][:, nodes], d["H"], d["normalized"]) for g, nodes in eigenpool_groups(d)}


EIG_GAP = 1e-3  # (fuzz_inputs.EIG_GAP: tests/test_fuzz_inputs.py asserts the two agree)


def eigenpool_compared_groups(d):
    """The groups whose entries are held by the rule -- one node, or, in float64, gaps of at least EIG_GAP among the
    used eigenvalues and a sign-fixing entry of at least EIG_GAP in every column, and a float32 restatement within
    CAP / FACTOR of it -- and the others, which keep the invariants of ``check_group_invariants`` alone."""
    from fuzz_compare import CAP, FACTOR
    m64, m32 = eigenpool_group_modes(d, torch.float64), eigenpool_group_modes(d, torch.float32)
    good, rest = [], []
    for g, nodes in eigenpool_groups(d):
        (want, lam), m = m64[g], nodes.numel()
        ok = m == 1
        if m > 1:
            used = min(d["H"] + 1, m)
            e32 = float(torch.linalg.vector_norm(m32[g][0].double() - want) / torch.linalg.vector_norm(want))
            ok = float((lam[1:used] - lam[:used - 1]).min()) >= EIG_GAP and float(want[0].abs().min()) >= EIG_GAP \
                and e32 <= CAP / FACTOR
        (good if ok else rest).append(g)
    return good, rest


def eigenpool_row_rank(gid):
    """int64 [n]: a row's place among the rows of its group, nodes ascending (the Reduce's order)."""
    order = torch.argsort(gid, stable=True)
    first = torch.zeros(int(gid.max()) + 2, dtype=torch.long)
    first[1:] = torch.bincount(gid).cumsum(0)
    rank = torch.empty_like(gid)
    rank[order] = torch.arange(gid.numel()) - first[gid[order]]
    return rank


def eigenpool_operator_reference(d, dtype, drop_row=None, late_wave=None, swap_modes=False):
    """"modes[g]" of every compared group, and on the Reduce's own inputs "pool" [G, H F] = sum over a group's rows of
    theta[i, h] x[i, f] and "lift" [n, F] = sum_h theta[i, h] y[gid_i, h F + f].  Wrong stand-ins: ``drop_row`` = k leaves
    the k-th row (from 1) of every group out of the Reduce; ``late_wave`` = W starts the second of W waves one row late
    (row ceil(len / W) of a group is lost); ``swap_modes`` exchanges the first two columns of every group's modes."""
    modes = eigenpool_group_modes(d, dtype)
    outs = {f"modes[{g}]": modes[g][0] for g in eigenpool_compared_groups(d)[0]}
    if swap_modes:
        outs = {k: (v[:, [1, 0] + list(range(2, v.size(1)))] if v.size(1) > 1 else v) for k, v in outs.items()}
    gid, G, H = d["reduce_gid"], d["reduce_groups"], d["reduce_H"]
    theta, x, y = d["theta"].to(dtype), d["reduce_x"].to(dtype), d["reduce_y"].to(dtype)
    keep = torch.ones(gid.numel(), dtype=dtype)
    rank, length = eigenpool_row_rank(gid), torch.bincount(gid, minlength=G)[gid]
    if drop_row is not None:
        keep = keep * (rank != drop_row - 1).to(dtype)
    if late_wave is not None:
        keep = keep * (rank != -(-length // late_wave)).to(dtype)
    terms = (theta * keep.view(-1, 1)).unsqueeze(2) * x.unsqueeze(1)
    outs["pool"] = torch.zeros(G, H, x.size(1), dtype=dtype).index_add_(0, gid, terms).view(G, -1)
    outs["lift"] = (theta.unsqueeze(2) * y.view(G, H, -1)[gid]).sum(1)
    return outs, {}


def eigenpool_reference(d, dtype):
    """EigenPooling through ``labels=``: ``eigenpool_restatement.collapsed`` -- "x_pool" [groups, H F] and "lift" on the
    compared groups and their nodes (the modes of the others are free up to a sign or a rotation), "adj" [B, K, K] with
    the pooler's default post-processing.  Leaf x."""
    x = _leaf(d["x"], dtype)
    res = REG.collapsed(x, d["edge_index"], d["edge_weight"], d["batch"], d["labels"], d["width"], d["H"], d["normalized"],
                        dtype=dtype)
    good = torch.tensor(eigenpool_compared_groups(d)[0])
    rows = torch.isin(d["gid"], good)
    return {"x_pool": res["x_pool"].reshape(-1, res["x_pool"].size(-1))[good], "lift": res["lift"][rows],
            "adj": res["adj"]}, {"x": x}


def eigenpool_exact(d):
    """theta_ptr and theta_perm of the compact pooling matrix, and S as one-hot labels."""
    res = REG.collapsed(d["x"], d["edge_index"], d["edge_weight"], d["batch"], d["labels"], d["width"], 1, d["normalized"])
    return {"theta_ptr": res["theta_ptr"], "theta_perm": res["theta_perm"],
            "s": torch.nn.functional.one_hot(d["labels"], d["width"]).float()}
