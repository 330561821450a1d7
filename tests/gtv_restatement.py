"""GTVConv restated (reference tgp/mp/gtvconv.py): loop-free torch, any dtype, differentiable.

With ``h = x @ weight``

    out_i = act((h_i + delta * sum_{e: row(e) = i, col(e) != i} gamma_e (h_col(e) - h_i) + bias) [* mask_i])
    d_e = ||h_row(e) - h_col(e)||_1,     gamma_e = w_e / max(d_e, eps)       (w_e = 1 without weights)

The reference builds the same numbers as a Laplacian: ``get_laplacian`` removes the self-loops, duplicate edges add, and
``flow="target_to_source"`` collects the sum at ``edge_index[0]`` from ``edge_index[1]``.  Its dense mode is this
expression over the nonzero entries of ``adj[b]`` (the diagonal of ``adj`` cancels between the degree and the entry).
"""
import torch

ACTS = {"identity": None, "relu": torch.relu, "elu": torch.nn.functional.elu, "tanh": torch.tanh}


def propagate(h, edge_index, edge_weight=None, bias=None, mask=None, delta=1.0, eps=1e-3, act=None):
    """The propagation of projected rows ``h`` [N, C]; edges that are self-loops or leave [0, N) are left out."""
    n = h.size(0)
    row, col = edge_index[0], edge_index[1]
    keep = (row != col) & (row >= 0) & (row < n) & (col >= 0) & (col < n)
    row, col = row[keep], col[keep]
    diff = h[col] - h[row]
    d = diff.abs().sum(dim=-1)
    gamma = 1.0 / d.clamp(min=eps)
    if edge_weight is not None:
        gamma = edge_weight.reshape(-1)[keep] * gamma
    out = h + delta * torch.zeros_like(h).index_add_(0, row, gamma.unsqueeze(-1) * diff)
    if bias is not None:
        out = out + bias
    if mask is not None:
        out = out * mask.reshape(-1, 1).to(out.dtype)
    return out if act is None else act(out)


def dense_edges(adj):
    """A dense ``adj`` [B, N, N] as an edge list of the flat B N nodes: (edge_index, weights), row-major order."""
    B, n, _ = adj.shape
    b, i, j = torch.nonzero(adj, as_tuple=True)
    return torch.stack([b * n + i, b * n + j]), adj[b, i, j]


def distances(h, edge_index):
    """(per non-loop edge the channel differences |h_ic - h_jc|, d_e)."""
    row, col = edge_index[0], edge_index[1]
    keep = row != col
    diff = (h[row[keep]] - h[col[keep]]).abs()
    return diff, diff.sum(-1)


def layer(x, weight, bias, edge_index, edge_weight=None, mask=None, delta=1.0, eps=1e-3, act="relu"):
    """The whole layer as the reference's ``forward`` sees it: a tensor whose last two sizes agree is a dense adjacency
    (output [B, N, C], ``mask`` applied), anything else an edge list (``mask`` ignored, as in the reference)."""
    fn = ACTS[act] if isinstance(act, str) else act
    h = x @ weight
    if edge_index.size(-1) == edge_index.size(-2):
        h = h.unsqueeze(0) if h.dim() == 2 else h
        adj = edge_index.unsqueeze(0) if edge_index.dim() == 2 else edge_index
        B, n, _ = adj.shape
        ei, w = dense_edges(adj)
        m = None if mask is None else mask.reshape(-1)
        return propagate(h.reshape(B * n, -1), ei, w, bias, m, delta, eps, fn).view(B, n, -1)
    return propagate(h, edge_index, edge_weight, bias, None, delta, eps, fn)
