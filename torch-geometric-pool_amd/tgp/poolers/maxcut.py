"""MaxCutPool (Abate & Bianchi, ICLR 2025; reference poolers/maxcut.py, select/maxcut_select.py).

Select is a ``TopkSelect`` over a score that a small GNN computes: ``initial_layer``, a stack of
``GCNConv(normalize=False)`` layers on the delta-GCN propagation matrix ``P = I - delta L_sym``, a row MLP and a final
``Linear(., 1)``.  With ``assign_all_nodes`` every dropped node then joins the kept node most of its assigned in-neighbours
belong to (``max_iter`` rounds, leftovers at random inside their graph).  Reduce and Connect are ``BaseReduce`` and
``SparseConnect`` on that assignment; the auxiliary loss is the cut ``s^T A s / vol`` per graph.

One layer in collapsed form, with ``z = h W^T``, the sum over the edges ``r -> i`` that are not self-loops, ``deg`` the
row sums by source without self-loops and ``dinv = deg^-1/2`` (inf -> 0):

    h'_i = act((1 - delta) [i < n_P] z_i + delta dinv_i sum_{r -> i} w_e dinv_r z_r + b),    n_P = max(edge_index) + 1

Device float32 inputs with an int64 ``[2, E]`` list take the native route (``tgp.functions.maxcut_score`` /
``maxcut_loss``, ``MaxCutSelect.assign``), which forms neither ``P`` nor anything of size ``E x C``.  Host
tensors, other dtypes, sparse connectivity, a width above the kernels' limit, an activation the kernels do not know, an
``edge_weight`` that requires grad and a list with a hub (``kernels.maxcut_score_has_hub``) take the composed form with
the same results.
"""
from __future__ import annotations

from typing import Optional, Union

import torch
from torch import Tensor

from .. import functions as Fn
from .. import kernels as K
from ..connect import SparseConnect
from ..lift import BaseLift
from ..nn import GCNConv
from ..reduce import BaseReduce
from ..select import SelectOutput, TopkSelect, _resolve_activation
from ..src import PoolingOutput, SRCPooling
from ..utils.losses import maxcut_loss
from ..utils.ops import connectivity_to_edge_index, delta_gcn_matrix, get_random_map_mask

_NATIVE_ACTS = {"identity": "identity", "none": "identity", "tanh": "tanh", "relu": "relu"}


def _activation(name: str):
    return (lambda v: v) if name.lower() in ("identity", "none") else _resolve_activation(name)


class MaxCutScoreNet(torch.nn.Module):
    r"""The score network of MaxCutPool: ``initial_layer = Linear(F, F)``, one ``GCNConv(normalize=False)`` + ``mp_act``
    per entry of ``mp_units`` on the :math:`\delta`-GCN matrix, ``Linear`` + ``mlp_act`` per entry of ``mlp_units``,
    ``final_layer = Linear(., 1)`` and ``act``.  Returns the scores ``[N, 1]``.  Parameter names are the reference's
    (``initial_layer``, ``mp_convs.{l}.lin.weight`` / ``.bias``, ``mlp.{l}``, ``final_layer``)."""

    def __init__(self, in_channels: int, mp_units: list = [32, 32, 32, 32, 16, 16, 16, 16, 8, 8, 8, 8],
                 mp_act: str = "tanh", mlp_units: list = [16, 16], mlp_act: str = "relu", act: str = "tanh",
                 delta: float = 2.0, **kwargs):
        super().__init__()
        self.initial_layer = torch.nn.Linear(in_channels, in_channels)
        self.mp_act, self.mlp_act, self.act = _activation(mp_act), _activation(mlp_act), _activation(act)
        # the names the kernels know (None: the composed form applies the callable)
        self._native_acts = tuple(_NATIVE_ACTS.get(a.lower()) for a in (mp_act, mlp_act, act))
        self.mp_convs = torch.nn.ModuleList()
        in_units = in_channels
        for out_units in mp_units:
            self.mp_convs.append(GCNConv(in_units, out_units, normalize=False, cached=False))
            in_units = out_units
        self.mlp = torch.nn.ModuleList()
        for out_units in mlp_units:
            self.mlp.append(torch.nn.Linear(in_units, out_units))
            in_units = out_units
        self.final_layer = torch.nn.Linear(in_units, 1)
        self.delta = delta

    def reset_parameters(self):
        for conv in self.mp_convs:
            conv.reset_parameters()
        for layer in self.mlp:
            layer.reset_parameters()
        self.final_layer.reset_parameters()

    def native_case(self, x: Tensor, edge_index, edge_weight: Optional[Tensor]) -> bool:
        """Do these inputs take the native route?"""
        if not (isinstance(edge_index, Tensor) and not edge_index.is_sparse and edge_index.dim() == 2
                and edge_index.size(0) == 2 and edge_index.dtype == torch.int64 and edge_index.is_cuda
                and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.size(0) > 0
                and self.initial_layer.weight.is_cuda and self.initial_layer.weight.dtype == torch.float32
                and x.size(1) == self.initial_layer.in_features and len(self.mp_convs) > 0
                and None not in self._native_acts):
            return False
        if edge_weight is not None and (edge_weight.dtype != torch.float32 or edge_weight.numel() != edge_index.size(1)
                                        or (edge_weight.requires_grad and torch.is_grad_enabled())):
            return False
        if any(c.out_channels > K.maxcut_max_width() or c.bias is None for c in self.mp_convs):
            return False
        if not K.maxcut_tail_fits(self.mp_convs[-1].out_channels, list(self.mlp) + [self.final_layer]):
            return False
        # a hub: one wave would add its whole group in every layer, the composed form's atomics spread it
        return not K.maxcut_score_has_hub(edge_index, x.size(0))

    def forward(self, x: Tensor, edge_index, edge_weight: Optional[Tensor] = None) -> Tensor:
        if self.native_case(x, edge_index, edge_weight):
            tail = [t for lin in list(self.mlp) + [self.final_layer] for t in (lin.weight, lin.bias)]
            mp_act, mlp_act, act = self._native_acts
            score = Fn.maxcut_score(x, edge_index, edge_weight, (self.initial_layer.weight, self.initial_layer.bias),
                                    [c.lin.weight for c in self.mp_convs], [c.bias for c in self.mp_convs], tail,
                                    self.delta, mp_act, mlp_act, act)
            return score.view(-1, 1)
        if edge_weight is None and x.dtype != torch.float32 and isinstance(edge_index, Tensor) and not edge_index.is_sparse:
            # (the reference's Laplacian makes float32 ones even in a float64 run, a 1e-8 artefact: unit weights of x's dtype)
            edge_weight = x.new_ones(edge_index.size(1))
        edge_index, edge_weight = delta_gcn_matrix(edge_index, edge_weight, delta=self.delta)
        x = self.initial_layer(x)
        for conv in self.mp_convs:
            x = self.mp_act(conv(x, edge_index, edge_weight))
        for layer in self.mlp:
            x = self.mlp_act(layer(x))
        return self.act(self.final_layer(x))


class MaxCutSelect(TopkSelect):
    r"""The select operator of MaxCutPool: :class:`MaxCutScoreNet` scores the nodes, a ``TopkSelect`` without a
    projection of its own keeps the best ``ceil(ratio * n)`` of every graph (by score, not by its magnitude), and with
    ``assign_all_nodes`` every other node is assigned to its nearest kept node.  The ``SelectOutput`` carries the scores
    of all nodes as ``so.scores``."""

    def __init__(self, in_channels: int, ratio: Union[int, float] = 0.5, assign_all_nodes: bool = True, max_iter: int = 5,
                 mp_units: list = [32, 32, 32, 32, 16, 16, 16, 16, 8, 8, 8, 8], mp_act: str = "tanh",
                 mlp_units: list = [16, 16], mlp_act: str = "relu", act: str = "tanh", delta: float = 2.0,
                 min_score: Optional[float] = None, s_inv_op: str = "transpose"):
        super().__init__(in_channels=None, ratio=ratio, min_score=min_score, act="identity", s_inv_op=s_inv_op)
        self.in_channels = in_channels
        self.mp_units, self.mp_act = mp_units, mp_act
        self.mlp_units, self.mlp_act = mlp_units, mlp_act
        self.score_act, self.delta = act, delta
        self.assign_all_nodes, self.max_iter = assign_all_nodes, max_iter
        self.score_net = MaxCutScoreNet(in_channels=in_channels, mp_units=mp_units, mp_act=mp_act, mlp_units=mlp_units,
                                        mlp_act=mlp_act, act=act, delta=delta)

    def reset_parameters(self):
        super().reset_parameters()
        if hasattr(self, "score_net"):
            self.score_net.reset_parameters()

    def assign(self, so: SelectOutput, edge_index: Tensor, weight: Optional[Tensor], batch: Optional[Tensor],
               max_iter: Optional[int] = None) -> SelectOutput:
        """``so.assign_all_nodes(adj=edge_index, weight=weight, max_iter=, batch=, closest_node_assignment=True)``.  A
        device int64 list runs the propagation rounds natively: int32 labels on two buffers, ``max_iter`` launches without
        a host wait in between (a round with nothing to do changes nothing), then one wait for "all assigned"; leftovers
        take ``get_random_map_mask`` and the relabelling is the composed routine's.  A list with a destination of more
        than ``kernels.MAXCUT_ASSIGN_MAX_GROUP`` in-edges takes the composed routine."""
        max_iter = self.max_iter if max_iter is None else max_iter
        kept, n = so.node_index, so.num_nodes
        if not (isinstance(edge_index, Tensor) and not edge_index.is_sparse and edge_index.is_cuda
                and edge_index.dtype == torch.int64 and edge_index.dim() == 2 and edge_index.size(0) == 2
                and kept.is_cuda and 0 < kept.numel() < n and max_iter > 0 and n < (1 << 31)):
            return so.assign_all_nodes(adj=edge_index, weight=weight, max_iter=max_iter, batch=batch,
                                       closest_node_assignment=True)
        if batch is None and K.maxcut_n_p_host(edge_index) != n:
            # (without a batch vector the composed routine sizes its result by the list, not by the selection)
            return so.assign_all_nodes(adj=edge_index, weight=weight, max_iter=max_iter, batch=batch,
                                       closest_node_assignment=True)
        if weight is not None and weight.size(0) != n:
            raise ValueError(f"Weight tensor size ({weight.size(0)}) must match the number of nodes ({n})")
        dev = edge_index.device
        by_dst = K.sag_edge_group(edge_index, n, by_destination=True)
        if by_dst.max_members > K.MAXCUT_ASSIGN_MAX_GROUP:
            # a hub: the one wave of its group would walk it once per distinct label
            return so.assign_all_nodes(adj=edge_index, weight=weight, max_iter=max_iter, batch=batch,
                                       closest_node_assignment=True)
        labels = torch.zeros(n, dtype=torch.int32, device=dev)
        labels[kept] = torch.arange(1, kept.numel() + 1, dtype=torch.int32, device=dev)
        row, _ = K._edge_rows(edge_index)
        labels = K.maxcut_assign_rounds(by_dst, row, labels, max_iter)
        mask = labels > 0
        target = kept[(labels.to(torch.long) - 1).clamp_(min=0)]
        if not bool(mask.all()):  # the one wait
            left = get_random_map_mask(kept, mask, batch)
            target = target.clone()
            target[left[0]] = left[1]
        cluster_index = torch.unique(target, return_inverse=True)[1]
        out = SelectOutput(cluster_index=cluster_index, s_inv_op=getattr(so, "s_inv_op", "transpose"), weight=weight,
                           _trusted=True)
        for name in so._extra_args:
            if hasattr(so, name):
                setattr(out, name, getattr(so, name))
        return out

    def forward(self, x: Tensor, edge_index=None, edge_weight: Optional[Tensor] = None, batch: Optional[Tensor] = None,
                **kwargs) -> SelectOutput:
        if edge_index is None:
            edge_index, edge_weight = torch.zeros(2, 0, dtype=torch.long, device=x.device), None
        edge_index, edge_weight = connectivity_to_edge_index(edge_index, edge_weight)
        scores = self.score_net(x, edge_index, edge_weight)  # [N, 1]
        so = super().forward(x=scores, batch=batch)
        if self.assign_all_nodes:
            so = self.assign(so, edge_index, scores.squeeze(-1), batch)
        setattr(so, "scores", scores.squeeze(-1))
        so._extra_args.add("scores")
        return so

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}(in_channels={self.in_channels}, ratio={self.ratio}, "
                f"assign_all_nodes={self.assign_all_nodes}, mp_units={self.mp_units}, mp_act='{self.mp_act}', "
                f"mlp_units={self.mlp_units}, mlp_act='{self.mlp_act}', act='{self.score_act}', delta={self.delta}, "
                f"max_iter={self.max_iter})")


class MaxCutPooling(SRCPooling):
    r"""MaxCutPool: the nodes are scored by a :math:`\delta`-GCN that is trained, through the auxiliary loss
    :math:`\mathbf{s}^\top \mathbf{A} \mathbf{s} / V`, to give neighbours opposite signs; the best-scoring
    ``ceil(ratio * n)`` nodes of every graph become the supernodes, every other node joins its nearest one
    (``assign_all_nodes``), and the pooled graph connects the supernodes whose groups are connected.

    Select: :class:`MaxCutSelect`; Reduce: ``BaseReduce``; Connect: ``SparseConnect``, always on the full assignment;
    Lift: ``BaseLift``.  ``forward`` returns the loss as ``{"maxcut_loss": loss_coeff * loss}``.  The ``"maxcut"`` alias
    of ``get_pooler`` is not registered (the alias set is pinned to the five hot-path poolers)."""

    def __init__(self, in_channels: int, ratio: Union[float, int] = 0.5, assign_all_nodes: bool = True,
                 max_iter: int = 5, loss_coeff: float = 1.0, mp_units: list = [32, 32, 32, 32], mp_act: str = "tanh",
                 mlp_units: list = [16, 16], mlp_act: str = "relu", act: str = "tanh", delta: float = 2.0,
                 lift: str = "precomputed", s_inv_op: str = "transpose", connect_red_op: str = "sum",
                 lift_red_op: str = "sum", remove_self_loops: bool = True, degree_norm: bool = False,
                 edge_weight_norm: bool = True):
        super().__init__(
            selector=MaxCutSelect(in_channels=in_channels, ratio=ratio, assign_all_nodes=assign_all_nodes,
                                  max_iter=max_iter, mp_units=mp_units, mp_act=mp_act, mlp_units=mlp_units,
                                  mlp_act=mlp_act, act=act, delta=delta, s_inv_op=s_inv_op),
            reducer=BaseReduce(),
            lifter=BaseLift(matrix_op=lift, reduce_op=lift_red_op),
            connector=SparseConnect(reduce_op=connect_red_op, edge_weight_norm=edge_weight_norm, degree_norm=degree_norm,
                                    remove_self_loops=remove_self_loops))
        self.in_channels, self.ratio = in_channels, ratio
        self.assign_all_nodes, self.max_iter, self.loss_coeff = assign_all_nodes, max_iter, loss_coeff
        self.mp_units, self.mp_act = mp_units, mp_act
        self.mlp_units, self.mlp_act = mlp_units, mlp_act
        self.act, self.delta = act, delta

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None, so: Optional[SelectOutput] = None,
                batch: Optional[Tensor] = None, lifting: bool = False, **kwargs):
        if lifting:
            if so is None:
                raise ValueError("SelectOutput (so) cannot be None for lifting")
            return self.lift(x_pool=x, so=so)
        x = x.unsqueeze(-1) if x.dim() == 1 else x
        so = self.select(x=x, edge_index=adj, edge_weight=edge_weight, batch=batch)
        loss = self.compute_loss(so.scores, adj, edge_weight, batch)
        if self.assign_all_nodes:
            fused = self.reduce_connect(x, adj, edge_weight, so, batch)  # batches of small graphs: ONE launch
            if fused is not None:
                x_pool, batch_pool, ei, ew = fused
                return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so, loss=loss)
        x_pool, batch_pool = self.reduce(x=x, so=so, batch=batch)
        full_so = so  # Connect always runs on the full assignment
        if not self.assign_all_nodes:
            edge_index, _ = connectivity_to_edge_index(adj, edge_weight)
            full_so = self.selector.assign(so, edge_index, None, batch, self.max_iter)
        ei, ew = self.connect(edge_index=adj, so=full_so, edge_weight=edge_weight, batch_pooled=batch_pool)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so, loss=loss)

    def compute_loss(self, scores: Tensor, adj, edge_weight: Optional[Tensor] = None,
                     batch: Optional[Tensor] = None) -> dict:
        edge_index, edge_weight = connectivity_to_edge_index(adj, edge_weight)
        return {"maxcut_loss": maxcut_loss(scores, edge_index, edge_weight, batch, "mean") * self.loss_coeff}

    @property
    def has_loss(self) -> bool:
        return True

    def extra_repr_args(self) -> dict:
        return {"loss_coeff": self.loss_coeff}


__all__ = ["MaxCutPooling", "MaxCutSelect", "MaxCutScoreNet"]
