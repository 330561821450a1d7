"""Adaptive Structure Aware Pooling (Ranjan et al., AAAI 2020; reference poolers/asap.py:21-267).

Select is a ``TopkSelect`` over a fitness that ASAP computes itself; Reduce and Connect are ``BaseReduce`` and the
induced-subgraph ``SparseConnect`` on the list with the remaining self-loops added.  The fitness, on edges ``j -> i``:

    x_q[i]   = max over i's in-edges of x_pool[src]                       (x_pool = x, or GNN(x) when a GNN is given)
    l_e      = leaky_relu(att([lin(x_q)[dst], x_pool[src]]))
    alpha    = softmax of l over each destination's in-edges              (+1e-16 in the denominator), then dropout
    x_new[i] = sum_e alpha_e x[src_e]
    fitness  = LEConv(F, 1)(x_new, edge_index, edge_weight)

Two routes compute it.  The composed one is the formulas above as torch operators, on any device and dtype.  The native
one (device float32 tensors; one autograd node for the attention and one for the score in training) never applies the
``F x F`` ``Linear`` and never forms anything of size ``E x F`` (``tgp.functions.asap_attention``, ``LEConv.score``;
DESIGN 4.20).  Edge weights get no gradient from the native nodes: a call that asks for one takes the composed form.
"""
from __future__ import annotations

import inspect
from typing import Callable, Optional, Union

import torch
import torch.nn.functional as F
from torch import Tensor

from .. import functions as Fn
from ..connect import SparseConnect
from ..leconv import LEConv
from ..lift import BaseLift
from ..reduce import BaseReduce
from ..select import SelectOutput, TopkSelect
from ..src import PoolingOutput, SRCPooling
from ..utils.ops import add_remaining_self_loops, connectivity_to_edge_index

_ACT_NAMES = {"linear": "identity", "identity": "identity", "none": "identity", "tanh": "tanh", "sigmoid": "sigmoid"}


def edge_softmax(score: Tensor, dst: Tensor, num_nodes: int) -> Tensor:
    """PyG's ``softmax`` over the entries that share a destination (the maximum is taken without a gradient)."""
    mx = score.new_zeros(num_nodes).scatter_reduce_(0, dst, score.detach(), reduce="amax", include_self=False)
    ex = (score - mx[dst]).exp()
    return ex / (ex.new_zeros(num_nodes).index_add_(0, dst, ex) + 1e-16)[dst]


class ASAPooling(SRCPooling):
    r"""ASAP pooling: every node's neighbourhood (with the node itself) is summarised by attention against its
    max-pooled "master query", the summaries are scored by :class:`~tgp.leconv.LEConv`, the best ``ceil(ratio * n)`` of
    every graph are kept with their summary gated by the score, and the induced subgraph is kept.

    ``GNN``: None, or a class built as ``GNN(in_channels, in_channels, **kwargs)`` and called as
    ``gnn(x=, edge_index=, edge_weight=)``; ``kwargs`` the class does not take are dropped.  ``dropout`` acts on the
    attention coefficients in training.  As in the reference, ``add_self_loops`` is only checked against
    ``remove_self_loops`` and reported by ``repr``.

    Device float32 inputs take the native route; host tensors, other dtypes, sparse connectivity and an ``edge_weight``
    that requires grad take the composed form with the same semantics.  The ``"asap"`` alias of
    ``get_pooler`` is not registered (the alias set is pinned to the five hot-path poolers)."""

    def __init__(self, in_channels: int, ratio: Union[float, int] = 0.5, GNN: Optional[torch.nn.Module] = None,
                 dropout: float = 0.0, negative_slope: float = 0.2, add_self_loops: bool = False,
                 nonlinearity: Union[str, Callable] = "sigmoid", lift: str = "precomputed",
                 s_inv_op: str = "transpose", connect_red_op: str = "sum", lift_red_op: str = "sum",
                 remove_self_loops: bool = True, degree_norm: bool = False, edge_weight_norm: bool = False, **kwargs):
        if remove_self_loops and add_self_loops:
            raise ValueError("remove_self_loops and add_self_loops cannot be both True")
        super().__init__(
            selector=TopkSelect(ratio=ratio, act=nonlinearity, s_inv_op=s_inv_op),
            reducer=BaseReduce(),
            lifter=BaseLift(matrix_op=lift, reduce_op=lift_red_op),
            connector=SparseConnect(remove_self_loops=remove_self_loops, reduce_op=connect_red_op,
                                    degree_norm=degree_norm, edge_weight_norm=edge_weight_norm))
        self.in_channels, self.ratio = in_channels, ratio
        self.negative_slope, self.dropout = negative_slope, dropout
        self.GNN, self.add_self_loops = GNN, add_self_loops
        # the activation the score kernel can fuse (None: any other callable / name goes through the selector's own)
        self._fused_act = (_ACT_NAMES.get(nonlinearity.lower()) if isinstance(nonlinearity, str)
                           else "identity" if nonlinearity is None else None)
        self.select_scorer = LEConv(in_channels, 1)
        self.lin = torch.nn.Linear(in_channels, in_channels)
        self.att = torch.nn.Linear(2 * in_channels, 1)
        if GNN is not None:
            # keep only the kwargs that are used in the GNN (signature works when __code__ is not available)
            try:
                params = set(inspect.signature(GNN).parameters.keys())
            except (ValueError, TypeError):
                params = set()
            self.gnn_intra_cluster = GNN(in_channels, in_channels, **{k: v for k, v in kwargs.items() if k in params})
        else:
            self.gnn_intra_cluster = None

    def reset_parameters(self):
        self.lin.reset_parameters()
        self.att.reset_parameters()
        self.select_scorer.reset_parameters()
        if self.gnn_intra_cluster is not None:
            self.gnn_intra_cluster.reset_parameters()
        super().reset_parameters()

    # ------------------------------------------------------------------------------------------------ the fitness
    def attention(self, x: Tensor, x_pool: Tensor, edge_index: Tensor, mask: Optional[Tensor] = None):
        """(alpha [E'], x_new [N, F]) in the composed form; ``mask`` [E'] multiplies alpha in place of the dropout."""
        n = x.size(0)
        src, dst = edge_index[0], edge_index[1]
        x_pool_j = x_pool[src]
        x_q = x_pool.new_zeros(n, x_pool.size(1)).scatter_reduce_(
            0, dst.view(-1, 1).expand_as(x_pool_j), x_pool_j, reduce="amax", include_self=False)
        x_q = self.lin(x_q)[dst]
        score = self.att(torch.cat([x_q, x_pool_j], dim=-1)).view(-1)
        alpha = edge_softmax(F.leaky_relu(score, self.negative_slope), dst, n)
        alpha = alpha * mask if mask is not None else F.dropout(alpha, p=self.dropout, training=self.training)
        x_new = x.new_zeros(n, x.size(1)).index_add_(0, dst, x[src] * alpha.view(-1, 1))
        return alpha, x_new

    def _native_case(self, x, x_pool, edge_index, edge_weight) -> bool:
        return bool(isinstance(edge_index, Tensor) and x.is_cuda and x.dtype == torch.float32 and x.size(0) > 0
                    and x_pool.is_cuda and x_pool.dtype == torch.float32 and x_pool.shape == x.shape
                    and self.lin.weight.dtype == torch.float32 and self.lin.weight.is_cuda
                    and self.select_scorer.native_case(x, edge_index, edge_weight))

    def fitness(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None,
                mask: Optional[Tensor] = None, act: Optional[str] = None):
        """(alpha, x_new, score [N]) on the list that already has its self-loops.  ``act`` None: the raw fitness; a name
        the native kernel knows ("identity", "tanh", "sigmoid"): that activation applied, fused on the native route."""
        x_pool = x
        if self.gnn_intra_cluster is not None:
            x_pool = self.gnn_intra_cluster(x=x, edge_index=edge_index, edge_weight=edge_weight)
        if self._native_case(x, x_pool, edge_index, edge_weight):
            if mask is None and self.training and self.dropout > 0:
                mask = F.dropout(torch.ones(edge_index.size(1), dtype=x.dtype, device=x.device), p=self.dropout)
            alpha, x_new, p = Fn.asap_attention(x, x_pool, edge_index, self.lin.weight, self.lin.bias, self.att.weight,
                                                self.att.bias, self.negative_slope, mask,
                                                self.select_scorer.projections())
            score = self.select_scorer.score(x_new, edge_index, edge_weight, act or "identity", p)
            return alpha, x_new, score
        alpha, x_new = self.attention(x, x_pool, edge_index, mask)
        score = self.select_scorer(x_new, edge_index, edge_weight).view(-1)
        if act in (None, "identity"):
            return alpha, x_new, score
        return alpha, x_new, torch.tanh(score) if act == "tanh" else torch.sigmoid(score)

    def _score_and_select(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], batch: Optional[Tensor]):
        """(x_new, SelectOutput).  Ratio mode with an activation the kernel knows: the activated score goes straight
        to the device selection, as SAGPooling's does."""
        sel = self.selector
        if (self._fused_act is not None and type(sel) is TopkSelect and sel.ratio is not None and x.is_cuda
                and x.dtype == torch.float32 and x.size(0) > 0 and self._so_cached is None):
            _, x_new, score = self.fitness(x, edge_index, edge_weight, act=self._fused_act)
            return x_new, sel._native_select(score, batch, x.size(0))
        _, x_new, score = self.fitness(x, edge_index, edge_weight)
        return x_new, self.select(x=score, batch=batch)

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None, so: Optional[SelectOutput] = None,
                batch: Optional[Tensor] = None, lifting: bool = False, **kwargs):
        if lifting:
            return self.lift(x_pool=x, so=so)
        n = x.size(0)
        x = x.unsqueeze(-1) if x.dim() == 1 else x
        edge_index, edge_weight = connectivity_to_edge_index(adj, edge_weight)
        edge_index, edge_weight = add_remaining_self_loops(edge_index, edge_weight, fill_value=1.0, num_nodes=n)
        # (a single graph is selected as one segment without a batch vector; Reduce and Connect get the reference's zeros)
        x_new, so = self._score_and_select(x, edge_index, edge_weight, batch)
        if batch is None:
            batch = edge_index.new_zeros(n)
        fused = self.reduce_connect(x_new, edge_index, edge_weight, so, batch)  # batches of small graphs: ONE launch
        if fused is not None:
            x_pool, batch_pool, ei, ew = fused
            return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)
        x_pool, batch_pool = self.reduce(x=x_new, so=so, batch=batch)
        ei, ew = self.connect(edge_index=edge_index, so=so, edge_weight=edge_weight, batch_pooled=batch_pool)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)

    def extra_repr_args(self) -> dict:
        return {"ratio": self.ratio, "GNN": self.GNN.__class__.__name__ if self.GNN is not None else "None",
                "add_self_loops": self.add_self_loops}


__all__ = ["ASAPooling", "LEConv"]
