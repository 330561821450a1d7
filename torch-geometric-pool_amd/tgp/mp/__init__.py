"""Message-passing layers (reference tgp/mp/gtvconv.py): ``GTVConv``, the layer of "Total Variation Graph Neural
Networks" (Hansen & Bianchi, ICML 2023) that the TVGNN model stacks in front of ``AsymCheegerCutPooling``.

With ``h = x @ weight`` the layer computes

    out_i = act((h_i + delta * sum_{e: row(e) = i, col(e) != i} gamma_e (h_col(e) - h_i) + bias) [* mask_i])
    d_e = ||h_row(e) - h_col(e)||_1,     gamma_e = w_e / max(d_e, eps)       (w_e = 1 without weights)

Self-loops drop out (the reference's Laplacian removes them; in the dense mode the diagonal cancels), duplicate edges
add, and the sum is collected at ``edge_index[0]`` from ``edge_index[1]`` (the reference's ``flow="target_to_source"``).
The dense mode is the same expression over the nonzero entries of ``adj[b]``; only it applies ``mask``, as in the
reference.

Routes.  Device float32 tensors take the native route (``tgp.functions.gtv_propagate``, csrc/gtvconv.hip): one launch per
forward, nothing of size E x C.  The dense mode runs on the same kernels: ``torch.nonzero(adj)`` is row-major in
(b, i, j), so it is a source-sorted edge list of the flat B N nodes whose by-source index is its CSR offsets alone.
Everything else takes ``gtv_propagate_composed`` (plain torch, the same edge order): host tensors, dtypes other than
float32, an ``edge_weight`` that is not a float32 vector, 2^31 edges or more, and -- in the dense mode -- an ``adj`` that
needs a gradient, which takes the matrix form of the reference (there the zero entries of ``adj`` receive a gradient,
which an edge walk does not produce).  ``tgp.kernels.gtv_record()`` tells which route served the last call.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import functions as Fn
from .. import kernels as K
from ..select import _resolve_activation
from ..utils.ops import connectivity_to_edge_index

__all__ = ["GTVConv", "gtv_adj_weights"]


def gtv_adj_weights(edge_index, edge_weight, num_nodes=None, flow="source_to_target", coeff=1.0):
    """``(edge_index, weights)`` of I - coeff L, L = D - A, over the list with a zero-weight loop added on every node that
    has none (reference mp/gtvconv.py:14-40); the degrees are summed at the destinations (``"source_to_target"``) or at
    the sources."""
    assert flow in ["source_to_target", "target_to_source"]
    row, col = edge_index[0], edge_index[1]
    n = num_nodes if num_nodes is not None else (int(edge_index.max()) + 1 if edge_index.numel() else 0)
    if edge_weight is None:
        edge_weight = torch.ones(edge_index.size(1), device=edge_index.device)
    # the non-loop edges in their order, then one loop per node: an existing loop keeps its weight, a new one gets 0
    keep = row != col
    loop = torch.arange(n, dtype=edge_index.dtype, device=edge_index.device)
    loop_w = edge_weight.new_zeros(n)
    loop_w[row[~keep]] = edge_weight[~keep]
    edge_index = torch.cat([edge_index[:, keep], loop.unsqueeze(0).repeat(2, 1)], dim=1)
    edge_weight = torch.cat([edge_weight[keep], loop_w])
    row, col = edge_index[0], edge_index[1]
    deg = edge_weight.new_zeros(n).index_add_(0, col if flow == "source_to_target" else row, edge_weight)
    on_diag = row == col
    edge_weight = -edge_weight
    edge_weight[on_diag] += deg
    edge_weight *= -coeff
    edge_weight[on_diag] += 1
    return edge_index, edge_weight


def gtv_propagate_composed(h: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None,
                           bias: Optional[Tensor] = None, mask: Optional[Tensor] = None, delta: float = 1.0,
                           eps: float = 1e-3, act=None) -> Tensor:
    """The propagation in plain torch, any device and dtype: the expression of the module docstring with one
    ``index_add`` in edge-list order.  Self-loops and edges with an end outside [0, N) are left out."""
    n = h.size(0)
    row, col = edge_index[0], edge_index[1]
    keep = (row != col) & (row >= 0) & (row < n) & (col >= 0) & (col < n)
    row, col = row[keep], col[keep]
    diff = h[col] - h[row]
    d = diff.abs().sum(dim=-1)
    gamma = 1.0 / d.clamp(min=eps)
    if edge_weight is not None:
        gamma = edge_weight.reshape(-1)[keep] * gamma
    msg = gamma.unsqueeze(-1) * diff  # (float64 weights on float32 rows promote, as torch's own arithmetic does)
    out = h + delta * torch.zeros(h.shape, dtype=msg.dtype, device=h.device).index_add_(0, row, msg)
    if bias is not None:
        out = out + bias
    if mask is not None:
        out = out * mask.reshape(-1, 1).to(out.dtype)
    return out if act is None else act(out)


def _gtv_dense_matrix_form(h: Tensor, adj: Tensor, bias, mask, delta: float, eps: float, act) -> Tensor:
    """The dense mode as a matrix product (reference mp/gtvconv.py:108-135), for an ``adj`` that needs a gradient: every
    entry of ``adj`` is a variable, the zero ones too (their scale is 1), which is what the reference differentiates."""
    B, Nn, _ = adj.shape
    b, i, j = torch.nonzero(adj, as_tuple=True)
    d = (h[b, i, :] - h[b, j, :]).abs().sum(dim=-1)
    scale = torch.ones_like(adj).index_put((b, i, j), 1.0 / d.clamp(min=eps))
    # the diagonal is left out: g_ii (h_i - h_i) is zero, and keeping a_ii / eps in both terms below would only cancel it
    # in floating point (the reference's own float32 error on graphs with self-loops)
    g = adj * scale * (1.0 - torch.eye(Nn, dtype=adj.dtype, device=adj.device))
    out = h + delta * (g @ h - g.sum(dim=-1, keepdim=True) * h)
    if bias is not None:
        out = out + bias
    if mask is not None:
        out = out * mask.view(B, Nn, 1).to(h.dtype)
    return out if act is None else act(out)


def _act_code(act) -> Optional[int]:
    """The forward kernel's code of ``act`` (None: a callable it does not know; torch applies it after the kernel)."""
    if act is None or type(act) is torch.nn.Identity:
        return K.GTV_ACT_CODES["identity"]
    if type(act) is torch.nn.ReLU:
        return K.GTV_ACT_CODES["relu"]
    if type(act) is torch.nn.ELU and act.alpha == 1.0:
        return K.GTV_ACT_CODES["elu"]
    return None


def _f32_on_device(*ts) -> bool:
    return all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in ts)


class GTVConv(torch.nn.Module):
    r"""The GTVConv layer (reference mp/gtvconv.py:43-170): one gradient-descent step on the graph total variation of
    the projected features, see the module docstring.

    Args:
        in_channels (int): size of the input node features.
        out_channels (int): size of the output node features.
        bias (bool): learn an additive bias (default ``True``).
        delta_coeff (float): step size of the descent (default ``1.0``).
        eps (float): floor of the distances that divide the edge weights (default ``1e-3``).
        act: activation: a name, a module or a callable (default ``"relu"``).
    """

    def __init__(self, in_channels: int, out_channels: int, bias: bool = True, delta_coeff: float = 1.0,
                 eps: float = 1e-3, act="relu"):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = torch.nn.Parameter(torch.empty(in_channels, out_channels))
        self.delta_coeff, self.eps = delta_coeff, eps
        # ("identity" is a name PyG's resolver knows and the package's table does not)
        self.act = torch.nn.Identity() if isinstance(act, str) and act.lower() == "identity" else _resolve_activation(act)
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.kaiming_normal_(self.weight)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def _propagate(self, h: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], mask: Optional[Tensor],
                   native: bool, by_src=None) -> Tensor:
        """One propagation over an edge list of the rows ``h`` [N, C] on the route chosen by the caller."""
        if not native:
            K.gtv_note("composed")
            return gtv_propagate_composed(h, edge_index, edge_weight, self.bias, mask, self.delta_coeff, self.eps,
                                          self.act)
        K.gtv_note("native")
        code = _act_code(self.act)
        fused = code is not None and (mask is None or mask.dtype == torch.bool)
        out = Fn.gtv_propagate(h.contiguous(), edge_index, edge_weight, self.bias, mask if fused else None,
                               self.delta_coeff, self.eps, code if fused else 0, by_src=by_src)
        if fused:
            return out
        if mask is not None:
            out = out * mask.reshape(-1, 1).to(out.dtype)
        return out if self.act is None else self.act(out)

    def forward(self, x: Tensor, edge_index, edge_weight: Optional[Tensor] = None, mask: Optional[Tensor] = None) -> Tensor:
        h = x @ self.weight
        C = h.size(-1)
        if isinstance(edge_index, Tensor) and not edge_index.is_sparse and edge_index.size(-1) == edge_index.size(-2):
            # a dense adjacency (the reference's own test: a [2, 2] edge list is read as one, too)
            h = h.unsqueeze(0) if h.dim() == 2 else h
            adj = edge_index.unsqueeze(0) if edge_index.dim() == 2 else edge_index
            B, Nn, _ = adj.size()
            if adj.requires_grad and torch.is_grad_enabled():
                K.gtv_note("composed")
                return _gtv_dense_matrix_form(h, adj, self.bias, mask, self.delta_coeff, self.eps, self.act)
            b, i, j = torch.nonzero(adj, as_tuple=True)  # row-major in (b, i, j): sorted by the flat source b N + i
            row, col = b * Nn + i, b * Nn + j
            ei, w = torch.stack([row, col]), adj[b, i, j]
            m = None if mask is None else mask.reshape(-1)
            native = (_f32_on_device(h, w, self.bias) and adj.is_cuda and (m is None or m.is_cuda) and h.size(0) == B
                      and 0 < B * Nn < 2 ** 31 and row.numel() < 2 ** 31 and C <= K.GTV_MAX_CHANNELS)
            by_src = None
            if native:
                ptr = torch.empty(B * Nn + 1, dtype=torch.int32, device=h.device)
                K.rowptr_from_sorted(row, B * Nn, ptr)
                by_src = K.AssignIndex(ptr, None, row.numel(), B * Nn)
            out = self._propagate(h.reshape(B * Nn, C), ei, w, m, native, by_src)
            return out.view(B, Nn, C)
        given = edge_weight
        edge_index, edge_weight = connectivity_to_edge_index(edge_index, edge_weight)
        native = (_f32_on_device(h, edge_weight, self.bias) and h.dim() == 2 and edge_index.is_cuda and h.size(0) > 0
                  and (given is None or given.dim() == 1) and edge_index.size(1) < 2 ** 31
                  and (edge_weight is None or edge_weight.numel() == edge_index.size(1))
                  and C <= K.GTV_MAX_CHANNELS)
        return self._propagate(h, edge_index, edge_weight, None, native)

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, delta_coeff={self.delta_coeff}, "
                f"eps={self.eps}, act={self.act})")
