"""One-channel graph convolutions: the scorers of :class:`~tgp.poolers.SAGPooling`.

``GraphConv`` and ``SAGEConv`` carry PyG's parameter names (``lin_rel`` / ``lin_root``, ``lin_l`` / ``lin_r``) and
``Linear`` initialisation, so a PyG checkpoint of a SAG layer loads unchanged.  Only what the pooler needs exists:
``out_channels == 1``, ``aggr`` "add" / "sum" / "mean", no edge weights -- anything else raises ``NotImplementedError``
naming the argument.  With one output channel projection and aggregation commute, so device float32 tensors take the
native project-then-aggregate scorer (``tgp.functions.sag_score``: one pass over x, E scalar gathers, no ``E x F`` or
``N x F`` temporary); host tensors and other dtypes take the composed form (gather, ``index_add_``, two ``Linear``s).

``GCNConv`` (any width, ``normalize=False`` only, not in ``__all__``) is the layer of MaxCutPool's score net: it carries
PyG's names (``lin.weight``, ``bias``) and initialisation, and its forward is the composed form of
``tgp.poolers.MaxCutScoreNet``, whose native route reads the parameters directly (``tgp.functions.maxcut_score``).
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import functions as Fn

_AGGR_MEAN = {"add": False, "sum": False, "mean": True}


def _check(name: str, out_channels: int, aggr: str) -> bool:
    if out_channels != 1:
        raise NotImplementedError(f"{name}: out_channels={out_channels} is not implemented (the pooling scorer has one "
                                  "output channel)")
    if not isinstance(aggr, str) or aggr not in _AGGR_MEAN:
        raise NotImplementedError(f"{name}: aggr={aggr!r} is not implemented (one of 'add', 'sum', 'mean')")
    return _AGGR_MEAN[aggr]


class _OneChannelConv(torch.nn.Module):
    """lin_nb(aggr_{j -> i} x_j) + lin_self(x_i); the subclasses name the two ``Linear``s as PyG does."""

    _nb: str
    _self: Optional[str]

    def __init__(self, in_channels: int, out_channels: int, aggr: str, root: bool, bias: bool):
        super().__init__()
        self._mean = _check(type(self).__name__, out_channels, aggr)
        self.in_channels, self.out_channels, self.aggr = in_channels, out_channels, aggr
        setattr(self, self._nb, torch.nn.Linear(in_channels, out_channels, bias=bias))
        if root:
            setattr(self, self._self, torch.nn.Linear(in_channels, out_channels, bias=False))

    def _linears(self):
        return getattr(self, self._nb), getattr(self, self._self, None)

    def reset_parameters(self):
        for lin in self._linears():
            if lin is not None:
                lin.reset_parameters()

    def score(self, x: Tensor, edge_index: Tensor, use_tanh: bool = False) -> Optional[Tensor]:
        """act(forward(x, edge_index)) as a vector [N] from the native scorer, or None when the inputs are not its case
        (host tensors, another dtype, non-tensor connectivity)."""
        nb, root = self._linears()
        if not (isinstance(edge_index, Tensor) and not edge_index.is_sparse and edge_index.dim() == 2
                and edge_index.size(0) == 2 and x.is_cuda and edge_index.is_cuda and x.dim() == 2
                and x.dtype == torch.float32 and nb.weight.dtype == torch.float32 and x.size(0) > 0
                and x.size(1) == self.in_channels):
            return None
        return Fn.sag_score(x, edge_index, nb.weight, None if root is None else root.weight, nb.bias, self._mean,
                            use_tanh)

    def forward(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None) -> Tensor:
        if edge_weight is not None:
            raise NotImplementedError(f"{type(self).__name__}: edge_weight is not implemented (SAGPooling scores without "
                                      "edge weights)")
        x = x.view(-1, 1) if x.dim() == 1 else x
        native = self.score(x, edge_index)
        if native is not None:
            return native.view(-1, 1)
        if not isinstance(edge_index, Tensor) or edge_index.is_sparse:
            from .utils.ops import connectivity_to_edge_index
            edge_index, _ = connectivity_to_edge_index(edge_index, None)
        nb, root = self._linears()
        src, dst = edge_index[0], edge_index[1]
        agg = torch.zeros_like(x).index_add_(0, dst, x[src])
        if self._mean:
            deg = torch.zeros(x.size(0), dtype=x.dtype, device=x.device).index_add_(
                0, dst, torch.ones(dst.numel(), dtype=x.dtype, device=x.device))
            agg = agg / deg.clamp(min=1).view(-1, 1)
        out = nb(agg)
        return out if root is None else out + root(x)

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, aggr={self.aggr}"


class GraphConv(_OneChannelConv):
    r"""PyG's ``GraphConv`` (Morris et al. 2019) at one output channel, without edge weights:
    :math:`\mathbf{W}_1 \mathbf{x}_i + \mathbf{W}_2 \sum_{j \to i} \mathbf{x}_j`.  Parameters ``lin_rel.weight`` [1,F],
    ``lin_rel.bias`` [1], ``lin_root.weight`` [1,F]."""

    _nb, _self = "lin_rel", "lin_root"

    def __init__(self, in_channels: int, out_channels: int, aggr: str = "add", bias: bool = True):
        super().__init__(in_channels, out_channels, aggr, True, bias)


class SAGEConv(_OneChannelConv):
    r"""PyG's ``SAGEConv`` (Hamilton et al. 2017) at one output channel:
    :math:`\mathbf{W}_1 \mathrm{mean}_{j \to i} \mathbf{x}_j + \mathbf{W}_2 \mathbf{x}_i`.  Parameters ``lin_l.weight``
    [1,F], ``lin_l.bias`` [1], ``lin_r.weight`` [1,F] (absent with ``root_weight=False``)."""

    _nb, _self = "lin_l", "lin_r"

    def __init__(self, in_channels: int, out_channels: int, aggr: str = "mean", root_weight: bool = True,
                 bias: bool = True):
        super().__init__(in_channels, out_channels, aggr, bool(root_weight), bias)
        self.root_weight = bool(root_weight)


class GCNConv(torch.nn.Module):
    r"""PyG's ``GCNConv`` as :class:`~tgp.poolers.MaxCutScoreNet` uses it: ``normalize=False``, so
    :math:`\mathbf{x}'_i = \sum_{j \to i} w_{ji} \mathbf{W} \mathbf{x}_j + \mathbf{b}` on the list as given (the caller
    brings the propagation matrix).  Parameters ``lin.weight`` [out, in] (glorot) and ``bias`` [out] (zeros), PyG's names.
    The score net's native route reads these parameters and never calls this forward; this is the composed form."""

    def __init__(self, in_channels: int, out_channels: int, improved: bool = False, cached: bool = False,
                 add_self_loops: Optional[bool] = None, normalize: bool = True, bias: bool = True):
        super().__init__()
        if normalize:
            raise NotImplementedError("GCNConv: normalize=True is not implemented (the MaxCut score net brings its own "
                                      "propagation matrix)")
        if improved or add_self_loops:
            raise NotImplementedError("GCNConv: improved / add_self_loops are not implemented (they belong to "
                                      "normalize=True)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.lin.weight)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None) -> Tensor:
        if not isinstance(edge_index, Tensor) or edge_index.is_sparse:
            from .utils.ops import connectivity_to_edge_index
            edge_index, edge_weight = connectivity_to_edge_index(edge_index, edge_weight)
        z = self.lin(x)
        msg = z[edge_index[0]]
        if edge_weight is not None:
            msg = msg * edge_weight.view(-1, 1).to(msg.dtype)
        out = torch.zeros_like(z).index_add_(0, edge_index[1], msg)
        return out if self.bias is None else out + self.bias

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}"


__all__ = ["GraphConv", "SAGEConv"]  # (SAGPooling's scorers; GCNConv is imported by name)
