"""PyG's ``PANConv`` and the reference's ``PANPooling`` restated in plain torch, dense per graph: the yardstick of the PAN
tests (float64 on the CPU; any device and float dtype).

PyG is not installed here, so this file states the convolution from its published behaviour.  The README's standing
caveat applies: the fixture is made by the reference's own ``PANPooling`` over the PyG stand-in, the MET matrix it is fed
comes from this restatement, and a shared misreading of a PyG leaf (``PANConv``'s normalisation, ``scatter``, ``topk``)
would pass both sides.

For ``PANConv(in_channels, out_channels, filter_size=L)`` with ``lin = Linear(in, out)`` and ``weight [L + 1]``:

* **A_t.**  ``A_t[dst, src]`` = how often the edge ``src -> dst`` occurs in the list.  Edge values are ignored, duplicate
  edges count with their multiplicity, self-loops are kept.
* **Series.**  ``tmp_0 = weight[0] I``, ``tmp_n = weight[n] (tmp_{n-1} @ A_t)``, ``S = sum_n tmp_n``: the coefficient of
  ``A_t^n`` is the running product ``c_n = prod_{i <= n} weight[i]``.
* **Stored pattern.**  Structural: ``(i, j)`` is stored iff some walk of length ``<= L`` joins them, whatever the value
  (a zero or cancelling weight keeps the entry); the diagonal is always stored.
* **Degree.**  ``deg_i`` = the number of stored entries of row ``i`` (a count, not a weighted sum); ``dinv = deg^-1/2``
  with ``inf -> 0``.
* **MET matrix.**  ``M_ij = (dinv_j S_ij) dinv_i``, multiplied in that order.
* **Output.**  ``out = lin(M @ x)``; the forward returns ``(out, M)``.

``PANPooling``: ``score = beta[0] (x . p) + beta[1] colsum(M)``, then PyG's ``topk`` selection, ``x_pool = multiplier *
score[kept] * x[kept]`` and the induced submatrix of ``M`` on the kept nodes.
"""
import torch

from sag_restatement import activate, select


def transposed_adjacency(edge_index, n, dtype, device=None):
    a = torch.zeros(n, n, dtype=dtype, device=device)
    if edge_index.numel():
        a.index_put_((edge_index[1], edge_index[0]), torch.ones(edge_index.size(1), dtype=dtype, device=device),
                     accumulate=True)
    return a


def met_dense_one(edge_index, weight, n):
    """(M [n, n] dense, pattern [n, n] bool, S, deg) of one graph in ``weight``'s dtype."""
    dtype, dev = weight.dtype, weight.device
    a = transposed_adjacency(edge_index, n, dtype, dev)
    eye = torch.eye(n, dtype=dtype, device=dev)
    tmp = weight[0] * eye
    s = tmp
    reach, pattern = eye > 0, eye > 0
    hop = (a != 0).to(torch.float64)
    for k in range(1, weight.numel()):
        tmp = weight[k] * (tmp @ a)
        s = s + tmp
        reach = (reach.to(torch.float64) @ hop) > 0
        pattern = pattern | reach
    deg = pattern.sum(dim=1).to(dtype)
    dinv = deg.pow(-0.5)
    dinv = torch.where(torch.isinf(dinv), torch.zeros_like(dinv), dinv)
    m = (dinv.view(1, -1) * s) * dinv.view(-1, 1)
    return m, pattern, s, deg


def met(edge_index, weight, n, batch=None):
    """(index [2, nnz] row-major sorted, values [nnz]) of the MET matrix; with ``batch`` (sorted) graph by graph."""
    if batch is None:
        m, pattern, _, _ = met_dense_one(edge_index, weight, n)
        index = pattern.nonzero().t().contiguous()
        return index, m[index[0], index[1]]
    sizes = torch.bincount(batch, minlength=int(batch.max()) + 1 if batch.numel() else 0).tolist()
    assert bool((batch[1:] >= batch[:-1]).all()), "the restatement takes a sorted batch vector"
    idx, val, lo = [], [], 0
    eb = batch[edge_index[0]]
    assert bool((eb == batch[edge_index[1]]).all()), "an edge between two graphs: restate the whole input as one graph"
    for g, size in enumerate(sizes):
        ei = edge_index[:, eb == g] - lo
        m, pattern, _, _ = met_dense_one(ei, weight, size)
        at = pattern.nonzero().t().contiguous()
        idx.append(at + lo)
        val.append(m[at[0], at[1]])
        lo += size
    return torch.cat(idx, 1), torch.cat(val)


def conv(x, edge_index, weight, lin_w, lin_b, batch=None):
    """(out, index, values) of PANConv's forward."""
    index, values = met(edge_index, weight, x.size(0), batch)
    agg = torch.zeros_like(x).index_add(0, index[0], values.view(-1, 1) * x[index[1]])
    out = agg @ lin_w.t()
    return (out if lin_b is None else out + lin_b), index, values


def raw_score(x, index, values, p, beta):
    score1 = (x * p).sum(dim=-1)
    score2 = torch.zeros(x.size(0), dtype=values.dtype, device=x.device).index_add(0, index[1], values)
    return beta[0] * score1 + beta[1] * score2


def pool(x, index, values, batch, p, beta, nonlinearity="tanh", ratio=0.5, min_score=None, multiplier=1.0, perm=None):
    """(raw score, activated score, kept nodes in supernode order, their weights, x_pool, pooled index, pooled values);
    ``perm`` overrides the selection.  The pooled matrix is the induced submatrix in the input's entry order, endpoints
    relabelled to the rank of the kept node in ascending node order."""
    b = batch if batch is not None else torch.zeros(x.size(0), dtype=torch.long, device=x.device)
    raw = raw_score(x, index, values, p, beta)
    score = activate(raw, b, nonlinearity, min_score)
    if perm is None:
        perm = select(score, b, ratio, min_score)
    weight = score[perm]
    x_pool = x[perm] * weight.view(-1, 1)
    rank = torch.full((x.size(0),), -1, dtype=torch.long, device=x.device)
    rank[torch.sort(perm).values] = torch.arange(perm.numel(), device=x.device)
    keep = (rank[index[0]] >= 0) & (rank[index[1]] >= 0)
    return (raw, score, perm, weight, x_pool * multiplier if multiplier != 1 else x_pool, rank[index[:, keep]],
            values[keep])
