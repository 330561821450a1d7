"""Edge-contraction selection restated in plain torch (no custom kernels): the yardstick of the EdgePool tests and, run
on device tensors, the composed-ops baseline of ``tools/bench_edgepool.py``.

It follows the reference's selector (select/edge_contraction_select.py) statement by statement:

* **Scores.**  ``raw[e] = x[row[e]].w[:F] + x[col[e]].w[F:] + b``; ``e = f(raw) + add_to_edge_score`` with ``f`` the
  softmax over the entries that share ``col[e]``, ``tanh`` or ``sigmoid``.
* **Order.**  Descending ``e`` with **ties to the lower edge position** (a stable sort; NaN first, ``-0`` ties with
  ``+0``).  The reference's ``argsort`` leaves ties open.
* **Matching.**  The reference's ``maximal_matching`` loop: every live directed entry offers its rank to both endpoints,
  an entry whose rank is the minimum at both endpoints is matched, entries that touch a matched node die.  ``(i, j)`` and
  ``(j, i)`` are two entries, a self-loop can match its node with itself, duplicates are distinct ranks.  (The
  reference's sentinel ``n * n`` is "no live entry" here: it only differs when there are more than ``n * n`` entries.)
* **Clusters.**  ``cluster[col[m]] = row[m]`` for each matched entry: the representative is the SOURCE, which may be
  the larger index; every other node represents itself; ids are the rank of the representative among all
  representatives (``torch.unique(..., return_inverse=True)``).
* **Weights.**  The matched entry's score for both members of its cluster, 1 for singletons.

Works on any device and float dtype.
"""
import torch

METHODS = ("softmax", "tanh", "sigmoid")


def raw_scores(x, edge_index, weight, bias):
    F = x.size(1)
    w = weight.reshape(-1).to(x.dtype)
    raw = (x @ w[:F])[edge_index[0]] + (x @ w[F:])[edge_index[1]]
    return raw if bias is None else raw + bias.reshape(-1).to(x.dtype)[0]


def segment_softmax(raw, index, n):
    """PyG's ``softmax(src, index, num_nodes=n)``: exp(src - max of the segment) / (sum of the segment + 1e-16)."""
    mx = torch.full((n,), float("-inf"), dtype=raw.dtype, device=raw.device).scatter_reduce(
        0, index, raw.detach(), reduce="amax", include_self=True)
    ex = (raw - mx[index]).exp()
    den = torch.zeros(n, dtype=raw.dtype, device=raw.device).index_add(0, index, ex) + 1e-16
    return ex / den[index]


def normalize(raw, edge_index, n, method, add):
    if method == "softmax":
        f = segment_softmax(raw, edge_index[1], n)
    elif method == "tanh":
        f = torch.tanh(raw)
    elif method == "sigmoid":
        f = torch.sigmoid(raw)
    else:
        f = method(raw, edge_index, n)  # a user callable, called as the reference calls it
    return f + add


def scores(x, edge_index, weight, bias, method="softmax", add=0.5):
    return normalize(raw_scores(x, edge_index, weight, bias), edge_index, x.size(0), method, add)


def stable_perm(e):
    return torch.argsort(e.reshape(-1), dim=0, descending=True, stable=True)


def rank_of(perm, m):
    rank = torch.empty(m, dtype=torch.long, device=perm.device)
    rank[perm] = torch.arange(m, device=perm.device)
    return rank


def matching(edge_index, n, perm=None, return_rounds=False):
    """bool [E]: the reference's ``maximal_matching`` for the priority order ``perm`` (None: list order).  The host reads
    one flag per round, as the reference does."""
    dev = edge_index.device
    row, col = edge_index[0], edge_index[1]
    m = row.numel()
    rank = torch.arange(m, device=dev) if perm is None else rank_of(perm, m)
    match = torch.zeros(m, dtype=torch.bool, device=dev)
    mask = torch.ones(m, dtype=torch.bool, device=dev)
    none = m  # "no live entry at this node"
    rounds = 0
    while bool(mask.any()):
        rounds += 1
        if rounds > n + 1:
            raise RuntimeError("edge-contraction restatement: no progress")
        live = torch.where(mask, rank, torch.full_like(rank, none))
        node_rank = torch.full((n,), none, dtype=torch.long, device=dev)
        node_rank = node_rank.scatter_reduce(0, row, live, reduce="amin", include_self=True)
        node_rank = node_rank.scatter_reduce(0, col, live, reduce="amin", include_self=True)
        edge_rank = torch.minimum(node_rank[row], node_rank[col])
        match = match | (mask & (rank == edge_rank))
        unmatched = torch.ones(n, dtype=torch.bool, device=dev)
        unmatched[row[match]] = False
        unmatched[col[match]] = False
        mask = mask & unmatched[row] & unmatched[col]
    return (match, rounds) if return_rounds else match


def clusters(edge_index, n, match):
    """(cluster long [n], k): matched pairs share the id of their SOURCE's rank among the representatives."""
    dev = edge_index.device
    rep = torch.arange(n, device=dev)
    rep[edge_index[1][match]] = edge_index[0][match]
    is_rep = rep == torch.arange(n, device=dev)
    ids = torch.cumsum(is_rep.to(torch.long), 0) - 1
    return ids[rep], int(is_rep.sum())


def weights(edge_index, n, match, e):
    w = torch.ones(n, dtype=e.dtype, device=e.device)
    w = w.index_put((edge_index[0][match],), e[match])
    return w.index_put((edge_index[1][match],), e[match])


def select(e, edge_index, n, perm=None):
    """(match bool [E], cluster [n], k, weight [n]) behind the scores ``e`` (``perm`` overrides their order)."""
    match = matching(edge_index, n, stable_perm(e.detach()) if perm is None else perm)
    cluster, k = clusters(edge_index, n, match)
    return match, cluster, k, weights(edge_index, n, match, e)


def pool(x, edge_index, weight, bias, method="softmax", add=0.5, perm=None):
    """Scores + selection + Reduce (S^T X with the weights as values) in the dtype of ``x``:
    (e, match, cluster, weight, x_pool).  ``perm`` replaces the order of the scores (a float64 run that must follow the
    float32 order)."""
    n = x.size(0)
    e = scores(x, edge_index, weight, bias, method, add)
    match, cluster, k, w = select(e, edge_index, n, perm)
    x_pool = torch.zeros(k, x.size(1), dtype=x.dtype, device=x.device).index_add(0, cluster, x * w.view(-1, 1))
    return e, match, cluster, w, x_pool


def sequential_greedy(edge_index, n, perm=None):
    """Walk the entries in priority order; take one when neither endpoint is matched yet.  bool [E] (host loop): the
    matching the parallel rounds must reproduce."""
    row, col = edge_index[0].tolist(), edge_index[1].tolist()
    taken = [False] * n
    match = torch.zeros(len(row), dtype=torch.bool)
    for e in (range(len(row)) if perm is None else perm.tolist()):
        if not taken[row[e]] and not taken[col[e]]:
            match[e] = True
            taken[row[e]] = taken[col[e]] = True
    return match
