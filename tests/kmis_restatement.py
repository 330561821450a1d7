"""k-MIS selection restated in plain torch (no custom kernels): the yardstick of the k-MIS tests and, run on device
tensors, the composed-ops baseline of ``tools/bench_kmis.py``.

It follows Bacciu et al. (AAAI 2023) as the reference implements it: heuristic-updated scores, a descending order with
**ties to the lower node index** (a stable sort), rounds of k hops of min-propagation of the ranks of the unmasked nodes
(every hop from the previous hop's values), k hops of mask propagation, and a cluster pass that hands every node to the
MIS node whose rank reached it.  Messages travel from ``row`` to ``col``.  Works on any device and float dtype.
"""
import torch


def k_sums(score, edge_index, order_k, heuristic):
    """(A^T + I)^k applied to ones ("greedy") or to the scores ("w-greedy"); one application is
    new[c] = old[c] + sum over the edges (r, c) of old[r], the old values on the right."""
    row, col = edge_index[0], edge_index[1]
    s = torch.ones_like(score) if heuristic == "greedy" else score.clone()
    for _ in range(order_k):
        s = s.index_add(0, col, s[row])
    return s


def updated_score(score, edge_index, order_k, heuristic):
    score = score.reshape(-1)
    if heuristic is None:
        return score
    return score / k_sums(score, edge_index, order_k, heuristic)


def stable_perm(updated):
    return torch.argsort(updated.reshape(-1), dim=0, descending=True, stable=True)


def rank_of(perm, n):
    rank = torch.empty(n, dtype=torch.long, device=perm.device)
    rank[perm] = torch.arange(n, device=perm.device)
    return rank


def _hop_min(v, row, col):
    return v.scatter_reduce(0, col, v[row], reduce="amin", include_self=True)


def _hop_max(v, row, col):
    return v.scatter_reduce(0, col, v[row], reduce="amax", include_self=True)


def mis_cluster(edge_index, order_k, perm, n, return_rounds=False):
    """(mis bool [n], cluster long [n]) for the priority order ``perm`` (None: node order).  The host reads one flag
    per round, as the reference does."""
    dev = edge_index.device
    row, col = edge_index[0], edge_index[1]
    rank = torch.arange(n, device=dev) if perm is None else rank_of(perm, n)
    mis = torch.zeros(n, dtype=torch.bool, device=dev)
    mask = mis.clone()
    rounds = 0
    while not bool(mask.all()):
        rounds += 1
        if rounds > n + 1:
            raise RuntimeError("k-MIS restatement: no progress")
        m = torch.where(mask, torch.full_like(rank, n), rank)
        for _ in range(order_k):
            m = _hop_min(m, row, col)
        mis = mis | (m == rank)
        f = mis.to(torch.long)
        for _ in range(order_k):
            f = _hop_max(f, row, col)
        mask = f.bool()
    m = torch.where(mis, rank, torch.full_like(rank, n))
    for _ in range(order_k):
        m = _hop_min(m, row, col)
    inv = torch.arange(n, device=dev) if perm is None else perm
    owner = inv[m.clamp(max=max(n - 1, 0))] if n else m  # node whose rank arrived
    ids = torch.cumsum(mis.to(torch.long), 0) - 1
    cluster = ids[owner] if n else owner
    if return_rounds:
        return mis, cluster, rounds
    return mis, cluster


def select(score, edge_index, order_k, heuristic, n):
    """(mis indices, cluster, updated score) of the whole selector behind the score."""
    upd = updated_score(score, edge_index, order_k, heuristic)
    mis, cluster = mis_cluster(edge_index, order_k, stable_perm(upd), n)
    return mis.nonzero().view(-1), cluster, upd


def pool(x, edge_index, edge_weight, batch, weight, bias, order_k, heuristic, reduce_none=False):
    """Linear scorer + selection + Reduce (S^T X with the scores as values) in the dtype of ``x``:
    (score, mis, cluster, x_pool)."""
    n = x.size(0)
    score = torch.sigmoid(x @ weight.t() + bias).view(-1)
    mis, cluster, _ = select(score.detach(), edge_index, order_k, heuristic, n)
    if reduce_none:
        x_pool = x[mis] * score[mis].view(-1, 1)
    else:
        x_pool = torch.zeros(mis.numel(), x.size(1), dtype=x.dtype, device=x.device).index_add(
            0, cluster, x * score.view(-1, 1))
    return score, mis, cluster, x_pool


def sequential_greedy(edge_index, order_k, perm, n):
    """Walk ``perm``; take a node unless an earlier pick lies within k hops (undirected graphs).  bool [n]."""
    adj = torch.zeros(n, n, dtype=torch.bool)
    adj[edge_index[0], edge_index[1]] = True
    adj = adj | adj.t() | torch.eye(n, dtype=torch.bool)
    reach = torch.eye(n, dtype=torch.bool)
    for _ in range(order_k):
        reach = (reach.float() @ adj.float()) > 0
    mis = torch.zeros(n, dtype=torch.bool)
    for v in (range(n) if perm is None else perm.tolist()):
        if not bool((reach[v] & mis).any()):
            mis[v] = True
    return mis


def reach_within(edge_index, order_k, n):
    """R[i, j]: j is reached from i by a walk of at most k edges (row -> col), i itself included."""
    adj = torch.zeros(n, n, dtype=torch.bool)
    adj[edge_index[0], edge_index[1]] = True
    adj = adj | torch.eye(n, dtype=torch.bool)
    reach = torch.eye(n, dtype=torch.bool)
    for _ in range(order_k):
        reach = (reach.float() @ adj.float()) > 0
    return reach
