"""``LEConv``: the local-extremum convolution (Ranjan et al., AAAI 2020) that scores the clusters of
:class:`~tgp.poolers.ASAPooling`.

It carries PyG's parameter names (``lin1.weight``, ``lin1.bias``, ``lin2.weight``, ``lin3.weight``, ``lin3.bias``) and
``Linear`` initialisation, so a PyG checkpoint of an ASAP layer loads unchanged.  What it computes is what PyG's CODE
computes (``message = (a_j - b_i) w_e`` with ``a = lin1(x)`` taken at the source and ``b = lin2(x)`` at the target):

    out_i = lin3(x_i) + sum_{e: dst(e) = i} w_e (lin1(x_src(e)) - lin2(x_i))

PyG's doc-string formula writes the two roles the other way round; the code is the authority.

``forward`` is the composed form (any device, dtype and channel count, with edge weights; also the route of an
``edge_weight`` that requires grad).  ``score`` is the native form at one output channel on device float32 tensors, one
autograd node under autograd: projection and aggregation commute, so with ``p1 = <x, w1>``,
``p2 = <x, w2>``, ``p3 = <x, w3>`` and ``W_i`` the summed weight of i's in-edges

    out_i = p3_i + b3 + sum_e w_e p1[src_e] + (b1 - p2_i) W_i

needs three scalars per node and E scalar gathers (``tgp.functions.asap_leconv_score``), nothing of size ``E x F``.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import functions as Fn


class LEConv(torch.nn.Module):
    def __init__(self, in_channels: int, out_channels: int, bias: bool = True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin1 = torch.nn.Linear(in_channels, out_channels, bias=bias)
        self.lin2 = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.lin3 = torch.nn.Linear(in_channels, out_channels, bias=bias)

    def reset_parameters(self):
        self.lin1.reset_parameters()
        self.lin2.reset_parameters()
        self.lin3.reset_parameters()

    def native_case(self, x: Tensor, edge_index, edge_weight: Optional[Tensor] = None) -> bool:
        """Device float32 tensors, a ``[2, E]`` list, one output channel and no gradient asked for the edge weights."""
        w = self.lin1.weight
        return bool(self.out_channels == 1 and isinstance(edge_index, Tensor) and not edge_index.is_sparse
                    and edge_index.dim() == 2 and edge_index.size(0) == 2 and edge_index.dtype == torch.int64
                    and x.is_cuda and edge_index.is_cuda and x.dim() == 2 and x.dtype == torch.float32
                    and w.dtype == torch.float32 and w.is_cuda and x.size(0) > 0 and x.size(1) == self.in_channels
                    and (edge_weight is None or (edge_weight.is_cuda and edge_weight.dtype == torch.float32
                                                 and edge_weight.dim() == 1))
                    and not Fn._needs_grad(edge_weight))

    def projections(self) -> Tensor:
        """[3, F]: the three weight rows the attend kernel projects a finished row on."""
        return torch.cat([self.lin1.weight, self.lin2.weight, self.lin3.weight], dim=0)

    def score(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None, act: str = "identity",
              p: Optional[Tensor] = None) -> Optional[Tensor]:
        """act(forward(x, edge_index, edge_weight)) as a vector [N] from the native scorer, or None when the inputs
        are not its case.  ``act``: "identity", "tanh" or "sigmoid".  ``p`` [3, N]: the projections of ``x`` on
        :meth:`projections` when the caller already has them (the attend kernel emits them)."""
        if not self.native_case(x, edge_index, edge_weight):
            return None
        return Fn.asap_leconv_score(x, edge_index, edge_weight, self.projections(), self.lin1.bias, self.lin3.bias,
                                    act, p)

    def forward(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None) -> Tensor:
        x = x.view(-1, 1) if x.dim() == 1 else x
        native = self.score(x, edge_index, edge_weight)
        if native is not None:
            return native.view(-1, 1)
        if not isinstance(edge_index, Tensor) or edge_index.is_sparse:
            from .utils.ops import connectivity_to_edge_index
            edge_index, edge_weight = connectivity_to_edge_index(edge_index, edge_weight)
        src, dst = edge_index[0], edge_index[1]
        msg = self.lin1(x)[src] - self.lin2(x)[dst]
        if edge_weight is not None:
            msg = msg * edge_weight.view(-1, 1)
        return msg.new_zeros(x.size(0), msg.size(1)).index_add_(0, dst, msg) + self.lin3(x)

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}"


__all__ = ["LEConv"]
