"""Pooling layers of the north-star path and the ``get_pooler`` factory
(reference tgp/poolers/{__init__,topk,sag,asap,graclus,ndp,diffpool,mincut,dmon,asym_cheeger_cut,hosc,bnpool,just_balance,edge_contraction,lapool}.py).

``get_pooler`` knows the five poolers named by the hot path: ``topk``, ``graclus``, ``ndp``, ``diff``,
``mincut`` (+ ``diff_u`` / ``mincut_u``).  Every other alias of the reference raises the same
``ValueError("Unknown pooler_name=...")`` an unknown name does.  ``DMoNPooling``, ``AsymCheegerCutPooling``,
``HOSCPooling``, ``BNPool``, ``JustBalancePooling``, ``EdgeContractionPooling``, ``LaPooling``, ``SAGPooling``, ``ASAPooling``
(``tgp/poolers/asap.py``), ``MaxCutPooling`` (``tgp/poolers/maxcut.py``), ``EigenPooling`` (``tgp/poolers/eigenpool.py``)
``NMFPooling`` (``tgp/poolers/nmf.py``) and ``SEPPooling`` (``tgp/poolers/sep.py``) are built and exported as classes;
their ``dmon`` / ``acc`` / ``hosc`` / ``bnpool`` / ``jb`` / ``edgepool`` / ``lap`` / ``sag`` / ``asap`` / ``maxcut`` /
``eigen`` / ``nmf`` / ``sep`` aliases are not registered yet.  The message-passing layer the TVGNN model puts in front of ``AsymCheegerCutPooling`` is ``tgp.mp.GTVConv``
(reference tgp/mp/gtvconv.py).
"""
from __future__ import annotations

import inspect
import weakref
from typing import Callable, List, Optional, Union

import torch
from torch import Tensor

from .. import functions as Fn
from .. import kernels as K
from .. import nn as _nn
from ..connect import DenseConnect, KronConnect, SparseConnect
from ..lift import BaseLift
from ..reduce import BaseReduce
from ..select import DPSelect, EdgeContractionSelect, GraclusSelect, KMISSelect, LaPoolSelect, MLPSelect, NDPSelect, SelectOutput, TopkSelect
from ..src import BasePrecoarseningMixin, DenseSRCPooling, PoolingOutput, SRCPooling, _Pooled
from ..utils.ops import batch_info, batched_negative_edge_sampling, is_dense_adj, negative_edge_sampling
from ..utils.losses import (
    _MinCutTermsFn,
    _native_f32,
    acc_loss_terms,
    acc_sparse_loss_terms,
    asym_norm_loss,
    cluster_loss,
    bnpool_rec_loss_terms,
    cluster_connectivity_prior_loss,
    kl_loss,
    sparse_bce_reconstruction_loss,
    weighted_bce_reconstruction_loss,
    _ho_cut_composed_dense,
    hosc_loss_terms,
    hosc_orthogonality_loss,
    hosc_sparse_loss_terms,
    sparse_ho_mincut_loss,
    unbatched_hosc_orthogonality_loss,
    dmon_loss_terms,
    entropy_loss,
    _jb_native,
    jb_loss_mean,
    link_pred_loss,
    mincut_loss,
    mincut_loss_terms,
    orthogonality_loss,
    sparse_link_pred_loss,
    sparse_mincut_loss,
    sparse_spectral_loss,
    sparse_totvar_loss,
    spectral_loss,
    totvar_loss,
    unbatched_asym_norm_loss,
    unbatched_cluster_loss,
    unbatched_entropy_loss,
    unbatched_orthogonality_loss,
)
from ..utils.ops import connectivity_to_edge_index, postprocess_adj_pool_dense
from ..functions import LossPair
from .asap import ASAPooling
from .maxcut import MaxCutPooling, MaxCutScoreNet, MaxCutSelect
from .eigenpool import EigenPoolConnect, EigenPoolLift, EigenPoolReduce, EigenPoolSelect, EigenPooling
from .nmf import NMFPooling, NMFSelect
from .pan import PANPooling
from .sep import SEPPooling, SEPSelect

import os as _os

# r6: batched dense poolers on a SPARSE input whose graphs are large and sparse take the un-padded rows route (no [B,N,N]
# adjacency): TGP_ROWS_ROUTE=0 keeps the densifying route; the density bound is entries / (N x longest graph)
_ROWS_ROUTE = _os.environ.get("TGP_ROWS_ROUTE", "1") != "0"
# (a number: THE bound; None: the measured default 0.03 + 8 / K, at most 0.3 -- the rows route costs E x K gathered floats,
#  the densifying route N x Nmax x K flops on the matrix cores plus two passes over the dense adjacency, so the break-even
#  density falls with K: K = 256 ties at 5.8 %, K <= 128 still wins at 11-29 %, profiles/r06_rows_route_crossover.txt)
_ROWS_ROUTE_DENSITY = float(_os.environ["TGP_ROWS_ROUTE_DENSITY"]) if "TGP_ROWS_ROUTE_DENSITY" in _os.environ else None


def _rows_route_density(k: int) -> float:
    if _ROWS_ROUTE_DENSITY is not None:
        return float(_ROWS_ROUTE_DENSITY)
    return min(0.3, 0.03 + 8.0 / max(int(k), 1))
# A/B switch (read once): 0 keeps the selector and the pooling as two autograd nodes in training
_FOLD_TRAINING = _os.environ.get("TGP_FOLD_TRAINING", "1") != "0"
# ... 0 densifies sparse inputs (to_dense_batch + to_dense_adj) in front of the fused inference call as before
_FOLD_SPARSE_INPUTS = _os.environ.get("TGP_FOLD_SPARSE_INPUTS", "1") != "0"
# ... 0 sends a dense adjacency that requires a gradient (the second level of a stacked model) to the operator route as
# before, instead of keeping it on the one-node training routes with the native dA (csrc/dense_adj_grad.hip)
_ADJ_GRAD = _os.environ.get("TGP_ADJ_GRAD", "1") != "0"


# =============================================================================== sparse poolers
class TopkPooling(SRCPooling):
    r"""Top-k pooling: keep the best-scoring ``ceil(ratio * n)`` nodes of every graph, gate their
    features by the score, keep the induced subgraph (reference poolers/topk.py:14-195)."""

    def __init__(self, in_channels: int, ratio: Union[int, float] = 0.5, min_score: Optional[float] = None,
                 multiplier: float = 1.0, nonlinearity: Union[str, Callable] = "tanh",
                 lift: str = "precomputed", s_inv_op: str = "transpose", connect_red_op: str = "sum",
                 lift_red_op: str = "sum", remove_self_loops: bool = True, degree_norm: bool = False,
                 edge_weight_norm: bool = False):
        super().__init__(
            selector=TopkSelect(in_channels=in_channels, ratio=ratio, min_score=min_score, act=nonlinearity,
                                s_inv_op=s_inv_op),
            reducer=BaseReduce(),
            lifter=BaseLift(matrix_op=lift, reduce_op=lift_red_op),
            connector=SparseConnect(reduce_op=connect_red_op, degree_norm=degree_norm,
                                    edge_weight_norm=edge_weight_norm, remove_self_loops=remove_self_loops))
        self.multiplier = multiplier

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None,
                so: Optional[SelectOutput] = None, batch: Optional[Tensor] = None,
                attn: Optional[Tensor] = None, lifting: bool = False, **kwargs):
        if lifting:
            return self.lift(x_pool=x, so=so)
        if self._one_node_training(x, edge_weight, attn):
            out = self._forward_one_node(x, adj, edge_weight, batch)
            if out is not None:
                return out
        so = self.select(x=x if attn is None else attn, batch=batch)
        fused = self.reduce_connect(x, adj, edge_weight, so, batch)  # batches of small graphs, inference: ONE launch
        if fused is not None:
            x_pool, batch_pool, ei, ew = fused
            if self.multiplier != 1:
                x_pool = self.multiplier * x_pool
            return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)
        x_pool, batch_pool = self.reduce(x=x, so=so, batch=batch)
        if self.multiplier != 1:
            x_pool = self.multiplier * x_pool
        ei, ew = self.connect(so=so, edge_index=adj, edge_weight=edge_weight, batch_pooled=batch_pool)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)

    def _one_node_training(self, x, edge_weight, attn) -> bool:
        """Training on device tensors in the selector's fused-score mode: the forward is the inference call and ONE
        autograd node carries the gradient to x and the projection (Fn.topk_pool_train)."""
        sel = self.selector
        return bool(_FOLD_TRAINING and attn is None and not self.cached and torch.is_grad_enabled()
                    and isinstance(x, Tensor) and x.is_cuda and x.dim() == 2 and x.size(0) > 0
                    and type(sel) is TopkSelect and sel.weight is not None and sel.min_score is None
                    and sel.ratio is not None and sel._fused_act is not None and type(self.reducer) is BaseReduce
                    and (x.requires_grad or sel.weight.requires_grad)
                    and not (edge_weight is not None and edge_weight.requires_grad)
                    and not torch.cuda.is_current_stream_capturing()
                    and K.topk_pool_bwd_fits(x, sel.weight))

    def _forward_one_node(self, x, adj, edge_weight, batch):
        sel = self.selector
        with torch.no_grad():
            so = self.select(x=x, batch=batch)
            if not so.is_sparse or so.num_supernodes == 0 or so.s._nnz() != so.num_supernodes:
                return None
            fused = self.reduce_connect(x, adj, edge_weight, so, batch)
            if fused is not None:
                x_pool, batch_pool, ei, ew = fused
            else:
                x_pool, batch_pool = self.reduce(x=x, so=so, batch=batch)
        index = so.s.indices()
        x_pool, values = Fn.topk_pool_train(x, sel.weight, x_pool, so.weight, index[0], index[1],
                                            sel._fused_act == "tanh")
        # S with the tracked values: what reads so.s downstream (Lift, a user's loss) reaches the projection through them
        so.s = torch.sparse_coo_tensor(index, values, so.s.size(), is_coalesced=True)
        so._hold_values(values)
        if self.multiplier != 1:
            x_pool = self.multiplier * x_pool
        if fused is None:
            ei, ew = self.connect(so=so, edge_index=adj, edge_weight=edge_weight, batch_pooled=batch_pool)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)

    def extra_repr_args(self) -> dict:
        return {"multiplier": self.multiplier}


class SAGPooling(SRCPooling):
    r"""Self-attention graph pooling (Lee et al., ICML 2019; reference poolers/sag.py:17-228): the nodes are scored by a
    one-channel graph convolution of ``attn`` (default: ``x``), the best ``ceil(ratio * n)`` of every graph are kept,
    their features gated by the score, the induced subgraph kept.  ``TopkSelect`` (without a projection of its own) +
    ``BaseReduce`` + ``SparseConnect`` + ``BaseLift``.  As in the reference, edge weights do not enter the score.

    ``GNN``: None (:class:`tgp.nn.GraphConv`), :class:`tgp.nn.GraphConv` / :class:`tgp.nn.SAGEConv` or their names
    ``"graphconv"`` / ``"sage"``; these score device float32 inputs natively (project, then aggregate: no ``E x F``
    temporary), with the activation fused in ratio mode when it is tanh or linear.  Any other class is built as
    ``GNN(in_channels, 1, **kwargs)`` and called as ``self.gnn(attn, adj)``, as the reference does.  ``kwargs`` the
    class does not take are dropped.

    The ``"sag"`` alias of ``get_pooler`` is not registered yet (the alias set is pinned to the five hot-path poolers)."""

    _GNN_NAMES = {"graphconv": _nn.GraphConv, "sage": _nn.SAGEConv}

    def __init__(self, in_channels: int, ratio: Union[float, int] = 0.5, GNN: Optional[torch.nn.Module] = None,
                 min_score: Optional[float] = None, multiplier: float = 1.0,
                 nonlinearity: Union[str, Callable] = "tanh", lift: str = "precomputed", s_inv_op: str = "transpose",
                 connect_red_op: str = "sum", lift_red_op: str = "sum", remove_self_loops: bool = True,
                 degree_norm: bool = False, edge_weight_norm: bool = False, **kwargs):
        super().__init__(
            selector=TopkSelect(ratio=ratio, min_score=min_score, act=nonlinearity, s_inv_op=s_inv_op),
            reducer=BaseReduce(),
            lifter=BaseLift(matrix_op=lift, reduce_op=lift_red_op),
            connector=SparseConnect(reduce_op=connect_red_op, degree_norm=degree_norm,
                                    edge_weight_norm=edge_weight_norm, remove_self_loops=remove_self_loops))
        if isinstance(GNN, str):
            if GNN.lower() not in self._GNN_NAMES:
                raise ValueError(f"Unknown GNN='{GNN}'. Available names: {list(self._GNN_NAMES)}")
            GNN = self._GNN_NAMES[GNN.lower()]
        gnn_cls = GNN or _nn.GraphConv
        # keep only the kwargs that are used in the GNN (signature works when __code__ is not available)
        try:
            params = set(inspect.signature(gnn_cls).parameters.keys())
        except (ValueError, TypeError):
            params = set()
        self.gnn = gnn_cls(in_channels, 1, **{k: v for k, v in kwargs.items() if k in params})
        self.multiplier = multiplier

    def reset_parameters(self):
        self.gnn.reset_parameters()
        super().reset_parameters()

    def _score_and_select(self, attn: Tensor, adj, batch: Optional[Tensor]) -> SelectOutput:
        sel = self.selector
        if (isinstance(self.gnn, (_nn.GraphConv, _nn.SAGEConv)) and type(sel) is TopkSelect and sel.min_score is None
                and sel.ratio is not None and sel._fused_act is not None and self._so_cached is None):
            # ratio mode, tanh or linear: the activation rides in the aggregate kernel and the score goes straight to the
            # device selection (under autograd the scorer is one graph node; so.weight reaches it through take_unique)
            score = self.gnn.score(attn, adj, sel._fused_act == "tanh")
            if score is not None:
                return sel._native_select(score, batch, attn.size(0))
        return self.select(x=self.gnn(attn, adj), batch=batch)

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None,
                so: Optional[SelectOutput] = None, batch: Optional[Tensor] = None,
                attn: Optional[Tensor] = None, lifting: bool = False, **kwargs):
        if lifting:
            return self.lift(x_pool=x, so=so)
        attn = x if attn is None else attn
        attn = attn.view(-1, 1) if attn.dim() == 1 else attn
        so = self._score_and_select(attn, adj, batch)
        fused = self.reduce_connect(x, adj, edge_weight, so, batch)  # batches of small graphs: ONE launch
        if fused is not None:
            x_pool, batch_pool, ei, ew = fused
            if self.multiplier != 1:
                x_pool = self.multiplier * x_pool
            return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)
        x_pool, batch_pool = self.reduce(x=x, so=so, batch=batch)
        if self.multiplier != 1:
            x_pool = self.multiplier * x_pool
        ei, ew = self.connect(edge_index=adj, so=so, edge_weight=edge_weight, batch_pooled=batch_pool)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)

    def extra_repr_args(self) -> dict:
        return {"multiplier": self.multiplier}


class GraclusPooling(BasePrecoarseningMixin, SRCPooling):
    r"""Graclus pooling: greedy pairwise matching, features summed per pair, edges coalesced
    (reference poolers/graclus.py:14-159)."""

    def __init__(self, lift: str = "precomputed", s_inv_op: str = "transpose", connect_red_op: str = "sum",
                 lift_red_op: str = "sum", cached: bool = False, remove_self_loops: bool = True,
                 degree_norm: bool = False, edge_weight_norm: bool = False):
        super().__init__(
            selector=GraclusSelect(s_inv_op=s_inv_op),
            reducer=BaseReduce(),
            lifter=BaseLift(matrix_op=lift, reduce_op=lift_red_op),
            connector=SparseConnect(reduce_op=connect_red_op, remove_self_loops=remove_self_loops,
                                    degree_norm=degree_norm, edge_weight_norm=edge_weight_norm),
            cached=cached)
        self.cached = cached

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None,
                so: Optional[SelectOutput] = None, batch: Optional[Tensor] = None, lifting: bool = False,
                **kwargs):
        if lifting:
            return self.lift(x_pool=x, so=so)
        so = self.select(edge_index=adj, edge_weight=edge_weight, num_nodes=x.size(0), batch=batch)
        fused = self.reduce_connect(x, adj, edge_weight, so, batch)  # batches of small graphs, inference: ONE launch
        if fused is not None:
            x_pool, batch_pool, ei, ew = fused
            return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)
        x_pool, batch_pool = self.reduce(x=x, so=so, batch=batch)
        ei, ew = self.connect(edge_index=adj, so=so, edge_weight=edge_weight, batch_pooled=batch_pool)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)

    def extra_repr_args(self) -> dict:
        return {"cached": self.cached}


class NDPPooling(BasePrecoarseningMixin, SRCPooling):
    r"""Node Decimation Pooling: spectral +-1 partition, keep one side, Kron-reduce the Laplacian
    (reference poolers/ndp.py:14-142)."""

    def __init__(self, lift: str = "precomputed", s_inv_op: str = "transpose", lift_red_op: str = "sum",
                 cached: bool = False):
        super().__init__(selector=NDPSelect(s_inv_op=s_inv_op), reducer=BaseReduce(),
                         lifter=BaseLift(matrix_op=lift, reduce_op=lift_red_op), connector=KronConnect(),
                         cached=cached)
        self.cached = cached

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None,
                so: Optional[SelectOutput] = None, batch: Optional[Tensor] = None, lifting: bool = False,
                **kwargs):
        if lifting:
            return self.lift(x_pool=x, so=so)
        so = self.select(edge_index=adj, edge_weight=edge_weight, batch=batch, num_nodes=x.size(0))
        x_pool, batch_pool = self.reduce(x=x, so=so, batch=batch)
        # batch: the Kron reduction is taken per graph (block-batched kernel); the reference's connector ignores it
        ei, ew = self.connect(edge_index=adj, so=so, edge_weight=edge_weight, batch=batch)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)

    def extra_repr_args(self) -> dict:
        return {"cached": self.cached}


class KMISPooling(BasePrecoarseningMixin, SRCPooling):
    r"""k-MIS pooling (Bacciu et al., AAAI 2023; reference poolers/kmis.py:15-246): a maximal k-independent set chosen by
    node score becomes the supernodes, every node joins the member that reaches it within ``order_k`` hops, features are
    summed per supernode weighted by the scores (``reduce_red_op=None``: the members' own rows times their scores),
    edges are coalesced.  ``KMISSelect`` + ``BaseReduce`` + ``SparseConnect`` + ``BaseLift``.

    Ties between equal scores go to the lower node index and the selection is a pure function of the inputs (see
    ``KMISSelect``); ``scorer="canonical"`` yields float32 scores (``so.s`` is float32 where the reference's is int64)
    and is refused together with ``score_heuristic="w-greedy"``.  Callable scorers and ``"first"`` / ``"last"`` are
    rejected by the selector's assertion, as in the reference.  ``cached=True`` needs a scorer without parameters."""

    def __init__(self, in_channels: Optional[int] = None, order_k: int = 1, scorer: str = "linear",
                 score_heuristic: Optional[str] = "greedy", force_undirected: bool = False, lift: str = "precomputed",
                 s_inv_op: str = "transpose", reduce_red_op: Optional[str] = "sum", connect_red_op: str = "sum",
                 lift_red_op: str = "sum", remove_self_loops: bool = True, degree_norm: bool = False,
                 edge_weight_norm: bool = False, cached: bool = False):
        super().__init__(
            selector=KMISSelect(in_channels=in_channels, order_k=order_k, scorer=scorer,
                                score_heuristic=score_heuristic, force_undirected=force_undirected, s_inv_op=s_inv_op),
            reducer=BaseReduce(),
            lifter=BaseLift(matrix_op=lift, reduce_op=lift_red_op),
            connector=SparseConnect(reduce_op=connect_red_op, remove_self_loops=remove_self_loops,
                                    degree_norm=degree_norm, edge_weight_norm=edge_weight_norm),
            cached=cached)
        self.reduce_red_op = reduce_red_op
        self.cached = cached
        self.precoarsenable = scorer in ["random", "constant", "canonical", "degree"]
        if cached and scorer == "linear" or callable(scorer):
            raise Exception("Caching should be disabled when using a linear scorer or a callable scorer.")

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None,
                so: Optional[SelectOutput] = None, batch: Optional[Tensor] = None, lifting: bool = False,
                **kwargs):
        if lifting:
            return self.lift(x_pool=x, so=so)
        so = self.select(x=x, edge_index=adj, edge_weight=edge_weight, batch=batch)
        if self.reduce_red_op is None:
            x_pool = torch.index_select(x, index=so.mis, dim=-2) * so.weight[so.mis].view(-1, 1)
            batch_pool = None if batch is None else batch[so.mis]
        else:
            fused = self.reduce_connect(x, adj, edge_weight, so, batch)  # batches of small graphs: ONE launch
            if fused is not None:
                x_pool, batch_pool, ei, ew = fused
                return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)
            x_pool, batch_pool = self.reduce(x=x, so=so, batch=batch)
        ei, ew = self.connect(edge_index=adj, so=so, edge_weight=edge_weight, batch_pooled=batch_pool)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)

    def extra_repr_args(self) -> dict:
        return {"cached": self.cached}


class EdgeContractionPooling(SRCPooling):
    r"""Edge-contraction pooling (EdgePool: Diehl et al. 2019; Diehl 2019; Landolfi 2022; reference
    poolers/edge_contraction.py:15-185): every directed edge entry is scored from its two endpoint features, a maximal
    matching chosen greedily by descending score is contracted, features are summed per cluster weighted by the matched
    entry's score, edges are coalesced.  ``EdgeContractionSelect`` + ``BaseReduce`` + ``SparseConnect`` + ``BaseLift``.

    Ties between equal scores go to the lower edge position and the selection is a pure function of the inputs (see
    ``EdgeContractionSelect``)."""

    def __init__(self, in_channels: int, edge_score_method: Optional[Callable] = None, dropout: Optional[float] = 0.0,
                 add_to_edge_score: float = 0.5, lift: str = "precomputed", s_inv_op: str = "transpose",
                 connect_red_op: str = "sum", lift_red_op: str = "sum", remove_self_loops: bool = True,
                 degree_norm: bool = False, edge_weight_norm: bool = False):
        super().__init__(
            selector=EdgeContractionSelect(in_channels=in_channels, edge_score_method=edge_score_method, dropout=dropout,
                                           add_to_edge_score=add_to_edge_score, s_inv_op=s_inv_op),
            reducer=BaseReduce(),
            lifter=BaseLift(matrix_op=lift, reduce_op=lift_red_op),
            connector=SparseConnect(reduce_op=connect_red_op, remove_self_loops=remove_self_loops,
                                    degree_norm=degree_norm, edge_weight_norm=edge_weight_norm))

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None,
                so: Optional[SelectOutput] = None, batch: Optional[Tensor] = None, lifting: bool = False,
                **kwargs):
        if lifting:
            return self.lift(x_pool=x, so=so)
        edge_index, edge_weight = connectivity_to_edge_index(adj, edge_weight)
        so = self.select(x=x, edge_index=edge_index, batch=batch)
        fused = self.reduce_connect(x, edge_index, edge_weight, so, batch)  # batches of small graphs: ONE launch
        if fused is not None:
            x_pool, batch_pool, ei, ew = fused
            return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)
        x_pool, batch_pool = self.reduce(x=x, so=so, batch=batch)
        ei, ew = self.connect(edge_index=edge_index, so=so, edge_weight=edge_weight, batch_pooled=batch_pool)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)


# =============================================================================== dense poolers
class _DenseMLPPooling(DenseSRCPooling):
    """What DiffPool and MinCut share: MLPSelect + BaseReduce + DenseConnect wiring, the batched /
    unbatched control flow, and the optional block-diagonal sparse output."""

    def __init__(self, in_channels, k, act, dropout, remove_self_loops, degree_norm, edge_weight_norm,
                 adj_transpose, lift, s_inv_op, batched, sparse_output, cache_preprocessing):
        super().__init__(
            selector=MLPSelect(in_channels=in_channels, k=k, batched_representation=batched, act=act,
                               dropout=dropout, s_inv_op=s_inv_op),
            reducer=BaseReduce(),
            lifter=BaseLift(matrix_op=lift),
            connector=DenseConnect(remove_self_loops=remove_self_loops, degree_norm=degree_norm,
                                   adj_transpose=adj_transpose, edge_weight_norm=edge_weight_norm,
                                   sparse_output=sparse_output),
            adj_transpose=adj_transpose, cache_preprocessing=cache_preprocessing, batched=batched,
            sparse_output=sparse_output)

    # hooks filled in by the poolers -----------------------------------------------------
    # True: the operator route connects through self.connect (which caches, and records its own autograd graph); False:
    # through dense_connect, the loss on the raw S^T A S, then the post-processing
    _connects_through_operator = False

    def _batched_connect_and_loss(self, x, adj, so, mask, edge_weight, batch, batch_pooled, known_nodes=None):
        if self._connects_through_operator:
            adj_pool, _ = self.connect(edge_index=adj, so=so, edge_weight=edge_weight, batch=batch,
                                       batch_pooled=batch_pooled)
            return adj_pool, self._loss_from_fused(adj, so, mask, None, known_nodes=known_nodes)
        c = self.connector
        raw = c.dense_connect(adj=adj, s=so.s)
        loss = self._loss_from_fused(adj, so, mask, raw, known_nodes=known_nodes)
        adj_pool = postprocess_adj_pool_dense(raw, remove_self_loops=c.remove_self_loops,
                                              degree_norm=c.degree_norm, adj_transpose=c.adj_transpose,
                                              edge_weight_norm=c.edge_weight_norm)
        return adj_pool, loss

    def compute_sparse_loss(self, edge_index, edge_weight, S, batch) -> dict:
        raise NotImplementedError

    def _sparse_loss(self, edge_index, edge_weight, S, batch) -> dict:
        return self.compute_sparse_loss(edge_index, edge_weight, S, batch)

    # which auxiliary losses the pooler computes: "diff" (link + entropy), "mincut" (cut + ortho: their per-graph
    # terms come out of the pooling kernels), "dmon" (spectral + cluster + ortho from the raw S^T A S and their own
    # loss kernels), "acc" (total variation + balance from the adjacency and S alone, their own loss kernels), "hosc"
    # (first-order + motif cut and an orthogonality term: the raw S^T A S, the adjacency and S, their own loss kernels),
    # "bnpool" (reconstruction of the adjacency from S K S^T, its own tile kernels; a KL and a prior term as torch ops),
    # "jb" (Just Balance: the column norms of S alone, its own loss kernel; neither the adjacency nor S^T A S is read)
    _loss_kind = "diff"
    # kinds whose losses come from loss kernels of their own behind the operator route: the one-node training paths
    # (_SelectPoolSmallFn, _PoolLargeFn, _PoolUnbatchedFn, the sparse training node) and the rows route decline them
    # ("jb" declines the rows route only under autograd: in inference its loss kernel runs on the route's un-padded S)
    _LOSS_ONLY_KINDS = ("dmon", "acc", "hosc", "bnpool", "jb")

    # kinds whose losses walk the dense adjacency itself (ACC's total variation counts its nonzero entries, HOSC's motif
    # chain multiplies by it three times, BN-Pool's reconstruction loss meets every entry of it): they also decline the
    # one-launch sparse kernel, which never forms that adjacency in memory
    _DENSE_ADJ_LOSS_KINDS = ("acc", "hosc", "bnpool")

    @property
    def _loss_only(self) -> bool:
        return self._loss_kind in self._LOSS_ONLY_KINDS

    @property
    def _loss_reads_dense_adj(self) -> bool:
        return self._loss_kind in self._DENSE_ADJ_LOSS_KINDS

    @property
    def _mincut_terms(self) -> bool:
        return self._loss_kind in ("mincut",)

    @property
    def _wants_raw(self) -> bool:
        return self._loss_kind in ("mincut", "dmon", "hosc")

    def _fused_diff_scales(self, adj, known_nodes, adj_numel=None):
        """(link_scale, ent_scale) when the pooler's two losses can ride on the fused call (DiffPool, and only with the
        real-node count ``known_nodes`` the host already has).  ``adj_numel``: B * N * N of the padded adjacency when
        ``adj`` is not that tensor (sparse inputs), or a callable that gives it."""
        return None

    def _loss_from_fused(self, adj, so, mask, raw, terms=None, diff=None, known_nodes=None) -> dict:
        """The loss dict from what a fused route left: ``terms`` / ``diff`` when the route produced them, else the
        pooler's own loss on ``adj``, ``so`` and ``raw``."""
        raise NotImplementedError

    # the one-launch sparse kernel: what the pooler asks of the launch besides _wants_raw and _mincut_terms ...
    _sparse_diff_stats = False

    def _sparse_launch_loss(self, s, mask, raw, terms, stats, edges, info, num_nodes) -> dict:
        """... and the loss dict it makes of what came back.  ``stats``: the [B,4] records when ``_sparse_diff_stats``;
        ``edges`` = (edge_index, edge_weight, edge_ptr)."""
        raise NotImplementedError

    # the un-padded rows route: the loss mode of its native entries (1: MinCut's two terms, 2: DiffPool's two losses;
    # 0: no mode of theirs -- the staged operators and _rows_staged_loss, inference of the batched mode only); None: the
    # pooler does not take the route
    _rows_mode = None

    def _rows_staged_loss(self, s, ptr, max_nodes) -> dict:
        raise NotImplementedError

    def _pair_loss(self, both) -> dict:
        """The loss dict from the pooler's two finished batch means."""
        raise NotImplementedError

    def _lift(self, x, so, batch, batch_pooled):
        return self.lift(x_pool=x, so=so, batch=batch, batch_pooled=batch_pooled)

    # the gates the routes share (they take the submodules the route has looked up: a Module attribute costs a search)
    @staticmethod
    def _mlp_lins(sel):
        """The Linear layers of a selector that is exactly MLPSelect, else None."""
        return getattr(getattr(sel, "mlp", None), "lins", None) if type(sel) is MLPSelect else None

    @staticmethod
    def _single_linear(lins):
        """The only layer of ``_mlp_lins(sel)`` when there is exactly one and it is float32, else None."""
        if lins is None or len(lins) != 1:
            return None
        last = lins[0]
        return last if last.weight.dtype == torch.float32 else None

    def _plain_wiring(self, c) -> bool:
        return type(c) is DenseConnect and type(self.reducer) is BaseReduce

    @staticmethod
    def _padded_f32(x, adj, mask) -> bool:
        """A padded float32 device batch x [B,N,F], adj [B,N,N] with a bool mask or none."""
        return (isinstance(x, Tensor) and isinstance(adj, Tensor) and x.dim() == 3 and adj.dim() == 3 and x.is_cuda
                and x.dtype == torch.float32 and adj.dtype == torch.float32
                and (mask is None or mask.dtype == torch.bool) and adj.shape == (x.size(0), x.size(1), x.size(1)))

    @staticmethod
    def _adj_grad_ok(adj, c, handed: bool) -> bool:
        """May a one-node training route take this adjacency although it requires a gradient?  Only a dense adjacency
        the caller HANDED to forward() (one densified from an edge list would need the gradient at its E entries: the
        operator route), float32 and contiguous, without edge_weight_norm."""
        return bool(_ADJ_GRAD and handed and isinstance(adj, Tensor) and adj.dtype == torch.float32
                    and adj.is_contiguous() and not c.edge_weight_norm)

    @staticmethod
    def _flat_f32(x, edge_index, edge_weight, batch) -> bool:
        """An un-padded float32 device batch x [N,F], N > 0, with an int64 edge list [2,E], float32 edge weights or
        none, an int64 batch vector [N] or none."""
        return (isinstance(x, Tensor) and isinstance(edge_index, Tensor) and x.dim() == 2 and x.is_cuda
                and x.dtype == torch.float32 and x.size(0) > 0 and edge_index.dim() == 2 and edge_index.size(0) == 2
                and edge_index.dtype == torch.long and edge_index.is_cuda
                and (edge_weight is None or edge_weight.dtype == torch.float32)
                and (batch is None or (batch.dtype == torch.long and batch.numel() == x.size(0))))

    def _select_reduce_connect(self, x, adj, mask, want_batch=False, known_nodes=None):
        """Inference on a batch of small graphs with a single-Linear selector: Select + Reduce + Connect as ONE launch
        (tgp_dense_pool_select_f32: S is formed in the pooling kernel's registers and written once).  Returns a
        ``_Pooled`` (``terms``: MinCut's per-graph terms, ``diff``: DiffPool's two losses, ``batch_pool`` when
        ``want_batch``) or None when the case is not that one."""
        sel, c = self.selector, self.connector
        last = self._single_linear(self._mlp_lins(sel))
        if last is None or not self._plain_wiring(c) or not self._padded_f32(x, adj, mask):
            return None
        weight, bias = last.weight, last.bias
        if torch.is_grad_enabled() and (x.requires_grad or adj.requires_grad or weight.requires_grad
                                        or (bias is not None and bias.requires_grad)):
            return None
        if not K.dense_pool_is_small(x.size(0), x.size(1), weight.size(0), x.size(2)):
            return None
        flags = K.dense_flags(c.remove_self_loops, c.degree_norm, c.adj_transpose, c.edge_weight_norm)
        diff_scales = self._fused_diff_scales(adj, known_nodes)
        mincut = self._mincut_terms
        s, x_pool, raw, adj_pool, terms, *bp = K.dense_pool_select(
            x, adj, weight.detach(), None if bias is None else bias.detach(), mask, flags,
            want_raw=self._wants_raw, mincut_terms=mincut, want_batch=want_batch, diff_stats=diff_scales is not None)
        diff = None
        if diff_scales is not None:  # DiffPool (r6): both losses from the launch's per-graph records, one tail launch
            diff = K.diffpool_stats_tail(terms, diff_scales[0], diff_scales[1])
        return _Pooled(SelectOutput(s=s, s_inv_op=sel.s_inv_op, in_mask=mask), x_pool, raw, adj_pool,
                       terms if mincut else None, diff, bp[0] if want_batch else None)

    def _select_reduce_connect_sparse(self, x, edge_index, edge_weight, batch):
        """A sorted batch of small graphs that arrives as PyG hands it over (x [N,F], a row-sorted
        ``edge_index``): Select + Reduce + Connect + loss tails straight from the un-padded batch in ONE launch
        (tgp_dense_pool_select_sparse_f32: every graph's adjacency tile is built in LDS from its edges) -- neither
        ``to_dense_batch`` nor ``to_dense_adj`` runs and no [B,N,N] tensor exists.  Training takes the same launch as one
        autograd node (functions._SelectPoolSparseFn: the padded tensors the backward kernels read are side outputs).  Only
        for poolers whose losses do not walk the dense adjacency; returns a ``_Pooled`` with the finished ``loss`` or
        None."""
        sel, c = self.selector, self.connector
        last = self._single_linear(self._mlp_lins(sel))
        if (not _FOLD_SPARSE_INPUTS or self.cache_preprocessing or last is None or not self._plain_wiring(c)
                or not self._flat_f32(x, edge_index, edge_weight, batch)
                or batch is None  # (this route only: the kernel walks the graphs of a batch vector)
                or (edge_weight is not None and edge_weight.dim() != 1)):  # (this route only: one weight per edge)
            return None
        if self._loss_reads_dense_adj:
            return None  # (the batch is densified, as the reference does)
        weight, bias, grad = last.weight, last.bias, torch.is_grad_enabled()
        if grad and edge_weight is not None and edge_weight.requires_grad:
            return None  # (the edge weights get no gradient from the fused backward)
        training = grad and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad))
        if training and self._loss_only:
            return None  # (the loss-only kinds train on the operator route)
        # (a pooler whose losses need the dense adjacency -- DiffPool's link loss -- gets it as a side output of the launch)
        if training and not (_FOLD_TRAINING and not c.edge_weight_norm and K.mlp_select_bwd_fits(weight.size(0), x.size(1))):
            return None
        # the one-launch kernel walks every graph's edge range: the list must be grouped by ascending source node (what
        # PyG's loaders produce).  Known per tensor object once it has been looked at; a NEW list gets its ranges and
        # its verdict from one facts launch enqueued here, in front of the wait for the batch facts: the pooling kernel
        # is launched on the ranges at once and the verdict is read behind it (a list that fails it is remembered, the
        # outputs are dropped and the densified path below takes the call)
        known = K._rows_sorted_memo(edge_index) if edge_index.size(1) > 1 else True
        if known is False:
            return None
        pending = None
        if known is None:
            from ..utils.ops import prefetch_batch_info
            prefetch_batch_info(batch)
            pending = K.edge_facts_launch(edge_index, batch)
            if pending is None:
                return None
        info = batch_info(batch)  # (memoised per batch vector)
        if (not info.is_sorted
                or not K.dense_pool_is_small(info.num_graphs, info.max_nodes, weight.size(0), x.size(1))):
            if pending is not None:
                K.edge_facts_finish(pending, edge_index, info.ptr)  # (the launch is out: keep what it found)
            return None
        edge_ptr = pending[2] if pending is not None else K.graph_edge_ptr(edge_index, info.ptr)
        flags = K.dense_flags(c.remove_self_loops, c.degree_norm, c.adj_transpose, c.edge_weight_norm)
        mincut = self._mincut_terms
        if training:  # one autograd node; the padded tensors the backward reads are side outputs of the same launch
            diff_scales = None
            if not mincut:
                diff_scales = self._fused_diff_scales(None, x.size(0), info.num_graphs * info.max_nodes * info.max_nodes)
                if diff_scales is None:
                    if pending is not None:
                        K.edge_facts_finish(pending, edge_index, info.ptr)
                    return None
            s, mask, x_pool, raw, adj_pool, pair, bp = Fn.select_pool_sparse(
                x, weight, bias, edge_index, edge_weight, batch, info.ptr, edge_ptr, info.num_graphs,
                info.max_nodes, flags, self.adj_transpose, mincut, diff_scales, info.sizes)
            loss = self._pair_loss(pair)  # (both losses came with the fused call: a LossPair)
        else:  # the pooler's losses from what the launch wrote: no dense adjacency
            s, mask, x_pool, raw, adj_pool, terms, bp, *stats = K.dense_pool_select_sparse(
                x, edge_index, edge_weight, batch, info.ptr, edge_ptr, info.num_graphs, info.max_nodes,
                weight.detach(), None if bias is None else bias.detach(), flags, self.adj_transpose,
                want_raw=self._wants_raw, mincut_terms=mincut, diff_stats=self._sparse_diff_stats)
            loss = self._sparse_launch_loss(s, mask, raw, terms, stats[0] if stats else None,
                                            (edge_index, edge_weight, edge_ptr), info, x.size(0))
        if pending is not None and not K.edge_facts_finish(pending, edge_index, info.ptr):
            return None  # rows not sorted: what the kernel computed on clamped ranges is dropped
        so = SelectOutput(s=s, s_inv_op=sel.s_inv_op, in_mask=mask)
        so._graph_sizes = info.sizes
        return _Pooled(so, x_pool, raw if self._wants_raw else None, adj_pool, batch_pool=bp, loss=loss)

    def _select_reduce_connect_train(self, x, adj, mask, graph_sizes, want_batch=False, known_nodes=None,
                                     adj_handed=False):
        """Training on a batch of small graphs with a single-Linear selector: Select + Reduce + Connect + loss tails as
        ONE autograd node (functions._SelectPoolSmallFn: one forward launch, two backward launches; the selector and the
        pooling were two nodes with eight + one backward launches and an accumulation of the two gradients of X).
        ``adj_handed``: forward() was given this dense adjacency; one that requires a gradient then stays here and gets
        it from a launch behind the node's backward (:meth:`_adj_grad_ok`).
        Returns a ``_Pooled`` like :meth:`_select_reduce_connect`, the losses as a ``LossPair``."""
        sel, c = self.selector, self.connector
        last = self._single_linear(self._mlp_lins(sel))
        if (self._loss_only or last is None or not self._plain_wiring(c) or not self._padded_f32(x, adj, mask)
                or not torch.is_grad_enabled() or c.edge_weight_norm
                or (adj.requires_grad and not self._adj_grad_ok(adj, c, adj_handed))):
            return None
        weight, mincut = last.weight, self._mincut_terms
        if (not K.dense_pool_is_small(x.size(0), x.size(1), weight.size(0), x.size(2))
                or not K.mlp_select_bwd_fits(weight.size(0), x.size(2))):
            return None
        flags = K.dense_flags(c.remove_self_loops, c.degree_norm, c.adj_transpose, c.edge_weight_norm)
        diff_scales = self._fused_diff_scales(adj, known_nodes)
        s, x_pool, raw, adj_pool, pair, bp = Fn.select_pool_small(
            x, adj, weight, last.bias, mask, flags, mincut, mincut, diff_scales, graph_sizes, want_batch)
        return _Pooled(SelectOutput(s=s, s_inv_op=sel.s_inv_op, in_mask=mask), x_pool, raw if mincut else None, adj_pool,
                       pair if mincut else None, pair if diff_scales is not None else None, bp)

    def _select_reduce_connect_large(self, x, adj, mask, graph_sizes, so=None, symmetry=None, known_nodes=None,
                                     adj_handed=False):
        """Training on a padded batch whose graphs are beyond the one-wave kernels (C2-sized), r6: Select (single-Linear
        selector; otherwise ``so`` holds S) + Reduce + Connect + post-processing + the pooler's two losses as ONE
        autograd node (functions._PoolLargeFn: ~10 forward and ~13 backward launches where the operator-by-operator graph
        ran 65-71).  ``adj_handed``: as in :meth:`_select_reduce_connect_train` (the node's backward then also forms dA:
        one small product and one N^2 K launch).  Returns a ``_Pooled`` like :meth:`_select_reduce_connect_train`, or
        None."""
        sel, c = self.selector, self.connector
        if (not _FOLD_TRAINING or self._loss_only or not self._plain_wiring(c) or not self._padded_f32(x, adj, mask)
                or not torch.is_grad_enabled() or c.edge_weight_norm
                or (adj.requires_grad and not self._adj_grad_ok(adj, c, adj_handed))
                or x.size(0) == 0 or x.size(1) == 0 or x.size(2) == 0):  # (this route only: its grids need every extent)
            return None
        weight = bias = s = None
        if so is None:
            last = self._single_linear(self._mlp_lins(sel))
            if last is None:
                return None
            weight, bias = last.weight, last.bias
            k = weight.size(0)
            if not (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
                return None
        else:
            s = so.s
            if not (isinstance(s, Tensor) and s.dim() == 3 and s.dtype == torch.float32 and s.is_cuda
                    and s.shape[:2] == x.shape[:2] and (s.requires_grad or x.requires_grad)):
                return None
            k = s.size(2)
        if k == 0 or k > 4096 or K.dense_pool_is_small(x.size(0), x.size(1), k, x.size(2)):
            return None
        flags = K.dense_flags(c.remove_self_loops, c.degree_norm, c.adj_transpose, c.edge_weight_norm)
        mode, scales = 1, (0.0, 0.0)  # (the loss modes of the native entries: 1 MinCut's terms, 2 DiffPool's losses)
        if not self._mincut_terms:
            scales = self._fused_diff_scales(adj, known_nodes)
            if scales is None:
                return None
            mode = 2
        s_out, x_pool, raw, adj_pool, pair = Fn.pool_large(x, adj, weight, bias, mask, s, flags, mode, scales, graph_sizes,
                                                           symmetry() if callable(symmetry) else symmetry)
        if so is None:
            so = SelectOutput(s=s_out, s_inv_op=sel.s_inv_op, in_mask=mask)
        if mode == 1:
            return _Pooled(so, x_pool, raw, adj_pool, terms=pair)
        return _Pooled(so, x_pool, None, adj_pool, diff=pair)

    @staticmethod
    def _adj_symmetry(edge_index, edge_weight, dense_adj, batch):
        """kernels.AdjSymmetry for the adjacency forward() densified from this edge list, or None."""
        if not (isinstance(edge_index, Tensor) and edge_index.dim() == 2 and edge_index.size(0) == 2
                and edge_index.dtype == torch.long and edge_index.is_cuda and batch is not None
                and (edge_weight is None or isinstance(edge_weight, Tensor))):
            return None
        info = batch_info(batch)
        if not info.is_sorted or info.num_graphs != dense_adj.size(0):
            return None
        return K.AdjSymmetry(edge_index, edge_weight, dense_adj, batch, info.ptr)

    def _unbatched_fused(self, x, edge_index, edge_weight, batch, batched_out: bool = False):
        """Reduce, Connect and both auxiliary losses on the UN-padded rows, r6: ONE S^T [A S | X | S] product
        (tgp_segment_gemm_tn3_f32) behind the CSR SpMM -- the mincut numerator is trace(S_g^T (A S)_g), the link
        residual sum_e w_e^2 - 2 sum_g trace(raw_g) + sum_g |S_g^T S_g|^2 -- instead of per-edge dot products and
        index_add scatters (reference utils/losses.py:73-127, 204-240, 661-708; dense_conn.py:140-208;
        base_reduce.py:170-182): 40-45 launches -> ~10 per forward in the unbatched mode.  Under autograd the same
        forward is ONE autograd node (functions._PoolUnbatchedFn).

        ``batched_out`` (r6, late): the BATCHED poolers take the same route for a sparse input whose graphs are too
        large for the one-launch kernels and sparse enough (E <= d x N x longest graph, d = TGP_ROWS_ROUTE_DENSITY or the
        measured default 0.03 + 8 / K, at most 0.3):
        no [B,N,N] adjacency is ever built (reference src.py:374-452 densifies first; at the C2 shape that is 134 MB
        written and read three times per training step for 0.33 M entries).  The results are those of the batched mode:
        S^T A^T S when adj_transpose (= the transpose of S^T (A S); MinCut's degrees are then in-degrees, sum_i (A q)_i),
        S handed out padded [B,Nmax,K] with its mask, losses normalised as the batched forms do.

        Returns a ``_Pooled`` with x_pool [B,K,F], adj_pool [B,K,K], the pooled batch vector and the finished ``loss``;
        one with only ``so`` set when only Select could be done here (unbatched mode); None when the case is not this
        one."""
        c, sel = self.connector, self.selector
        mode = self._rows_mode
        grad = torch.is_grad_enabled()
        gate = self._rows_gate(x, edge_index, edge_weight, batch, batched_out, c, sel, mode, grad)
        if gate is None:
            return None
        info, ptr, max_nodes, nb, last = gate
        plan = self._rows_selector_plan(x, batch, batched_out, c, last, mode, grad)
        if plan is None or isinstance(plan, _Pooled):
            return plan
        ei, w_used, row_ptr, sw2, scales = self._rows_adjacency(x, edge_index, edge_weight, batched_out, mode, info, nb,
                                                                max_nodes)
        transposed = bool(batched_out and self.adj_transpose)
        flags = K.dense_flags(c.remove_self_loops, c.degree_norm, c.adj_transpose if batched_out else False,
                              c.edge_weight_norm)
        so, s_flat, x_pool, adj_pool, both_or_loss = self._rows_execute(
            x, edge_index, edge_weight, batch, batched_out, plan, mode,
            (row_ptr, ei, w_used, ptr, max_nodes, transposed, flags, mode, scales, sw2))
        return self._rows_hand_out(sel, so, s_flat, x_pool, adj_pool, both_or_loss, mode, batch, batched_out, info, nb,
                                   max_nodes)

    def _rows_gate(self, x, edge_index, edge_weight, batch, batched_out, c, sel, mode, grad):
        """Everything the rows route decides before Select runs: (info, ptr, max_nodes, number of graphs, the selector's
        single Linear or None), or None when the case is not this route's (nothing has been run or remembered then)."""
        staged = mode == 0  # (no loss mode in the native entries: the staged operators, see _rows_mode)
        if (mode is None or not self._plain_wiring(c) or (self.sparse_output and not batched_out)
                # (this route only: a non-tensor weight declines here instead of raising)
                or (edge_weight is not None and not isinstance(edge_weight, Tensor))
                or not self._flat_f32(x, edge_index, edge_weight, batch)
                # (this route only: the CSR and the products need an edge and a feature; the weights may have any shape)
                or edge_index.size(1) == 0 or x.size(1) == 0
                or (edge_weight is not None and edge_weight.numel() != edge_index.size(1))):
            return None
        if grad and edge_weight is not None and edge_weight.requires_grad:
            return None
        if staged and (not batched_out
                       or (grad and (x.requires_grad or any(p.requires_grad for p in sel.parameters())))):
            return None  # (such a pooler trains, and runs its unbatched mode, on the operator route)
        n = x.size(0)
        info = None
        if batch is not None:
            info = batch_info(batch)
            if not info.is_sorted:
                return None
            ptr, max_nodes, nb = info.ptr, info.max_nodes, info.num_graphs
        else:
            ptr, max_nodes, nb = Fn._whole_range(n, x.device), n, 1
        lins = self._mlp_lins(sel)
        if batched_out:  # every check comes BEFORE Select here: a bail-out must leave the batched flow untouched
            w_out = None if lins is None else lins[-1].weight  # (K is the last layer's, however many there are)
            if (not _ROWS_ROUTE or self.cache_preprocessing or w_out is None or w_out.dtype != torch.float32
                    or edge_index.size(1) > _rows_route_density(w_out.size(0)) * float(n) * float(max_nodes)
                    or K.dense_pool_is_small(nb, max_nodes, w_out.size(0), x.size(1))):
                return None
            will_train = grad and (x.requires_grad or any(p.requires_grad for p in sel.parameters()))
            if will_train and (not _FOLD_TRAINING or c.edge_weight_norm or w_out.size(0) > 4096):
                return None
        return info, ptr, max_nodes, nb, self._single_linear(lins)

    def _rows_select(self, x, batch, batched_out):
        """(so, S [N,K]) of the selector run on its own on the un-padded rows."""
        so = self.select(x=x, batch=batch) if not batched_out else self.select(x=x)
        s = so.s
        if batched_out and isinstance(s, Tensor) and s.dim() == 3 and s.size(0) == 1:
            s = s[0]  # (MLPSelect in its batched representation treats [N,F] as one padded graph)
        return so, s

    def _rows_selector_plan(self, x, batch, batched_out, c, last, mode, grad):
        """What becomes of the selector: (weight, bias, s, so, training) -- ``weight`` / ``bias`` of its single Linear when
        it is folded into the one native call of the inference or into the training node (``s`` and ``so`` are None
        then), else the S and the SelectOutput of the selector run in front.  The route's own answer when it stops here:
        None, or -- unbatched mode -- a ``_Pooled`` with only ``so`` (the caller goes on with it on the operator path)."""
        so = s = weight = bias = None
        w, b = (last.weight, last.bias) if last is not None else (None, None)
        if (w is not None and not grad and K._POOL_ROWS_ONE_CALL and x.dtype == torch.float32 and x.is_contiguous()
                and w.size(0) <= 256 and mode != 0):
            # inference with a single-Linear selector (r6, late): the selector rides in the ONE native call of the forward
            # (kernels.pool_rows_forward); the SelectOutput is built from the S it leaves
            weight, bias, training = w.detach(), None if b is None else b.detach(), False
        elif w is not None and grad and _FOLD_TRAINING:  # a single Linear: folded into the training node, if anything trains
            training = x.requires_grad or w.requires_grad or (b is not None and b.requires_grad)
            if training:
                weight, bias = w, b
            else:
                so, s = self._rows_select(x, batch, batched_out)
        else:  # the selector runs in front: its S is handed over
            so, s = self._rows_select(x, batch, batched_out)
            if not (isinstance(s, Tensor) and s.dim() == 2 and s.dtype == torch.float32 and s.size(0) == x.size(0)):
                return None if batched_out else _Pooled(so)  # (the caller goes on with it on the operator path)
            training = grad and (s.requires_grad or x.requires_grad)
        k = s.size(1) if s is not None else weight.size(0)
        if training and (not _FOLD_TRAINING or c.edge_weight_norm or k > 4096):
            if batched_out:
                return None
            return _Pooled(so if so is not None else self._rows_select(x, batch, False)[0])
        return weight, bias, s, so, training

    def _rows_adjacency(self, x, edge_index, edge_weight, batched_out, mode, info, nb, max_nodes):
        """(ei, weights or None when all are one, CSR offsets, sw2, scales): the sorted, duplicate-summed A (what the
        reference's per-graph ``.coalesce()`` does) and, for DiffPool, sum_e w_e^2 with the two loss scales."""
        n = x.size(0)
        w_in = None if edge_weight is None else edge_weight.reshape(-1)
        ones = w_in is None
        if ones and K.coalesced_memo(edge_index, n):  # (known to be coalesced: no vector of ones is made for the check)
            ei, w = edge_index, None
        else:
            ei, w = Fn.coalesce_sum(edge_index, torch.ones(edge_index.size(1), device=x.device) if ones else w_in.detach(), n)
        unit = ones and ei is edge_index  # (nothing merged: the weights are still all one)
        row_ptr = K.csr_offsets(ei, n)
        sw2, scales = 0.0, (0.0, 0.0)
        if mode == 2:  # the link loss: sum_e w_e^2 runs over the list as given (duplicates not merged, losses.py:680-690)
            # (batched form, losses.py:644-652: the dense A has the duplicates summed -- the same list after coalescing)
            if batched_out and not unit:
                sw2 = torch.dot(w, w)
            else:
                sw2 = float(edge_index.size(1)) if ones else torch.dot(w_in.detach(), w_in.detach())
            # (the normaliser, asked only when the link loss is normalised: adj.numel() of the padded batch, losses.py:651)
            scales = self._fused_diff_scales(None, n, (lambda: nb * max_nodes * max_nodes) if batched_out else (
                lambda: sum(v * v for v in info.sizes_host) if info is not None else n * n))
        return ei, None if unit else w, row_ptr, sw2, scales

    def _rows_execute(self, x, edge_index, edge_weight, batch, batched_out, plan, mode, args):
        """Reduce, Connect and the losses by exactly one of the training node, the staged operators (``mode`` 0) and the
        native forward; ``args``: kernels.pool_rows_forward's behind S.  Returns (so, S [N,K], x_pool, adj_pool, the
        pooler's two batch means -- the finished loss dict from the staged operators)."""
        weight, bias, s, so, training = plan
        row_ptr, ei, w_used, ptr, max_nodes, transposed, flags, _, scales, sw2 = args
        if training:
            sym = K.AdjSymmetry.of_edge_list(edge_index, edge_weight, ei, w_used, row_ptr, x.size(0))
            s, x_pool, _, adj_pool, both = Fn.pool_unbatched(x, weight, bias, s, ei, w_used, row_ptr, ptr, batch, max_nodes,
                                                             flags, mode, scales, sw2, sym, transposed)
            return so, s, x_pool, adj_pool, both
        if mode == 0:  # T = A S, S^T [T | X] with the post-processing, the pooler's loss on the un-padded S
            t = K.spmm_csr(row_ptr, ei, w_used, x.size(0), s)
            _, x_pool, adj_pool = K.segment_gemm_tn3(s, [t, x], ptr, max_nodes, transpose0=transposed, post_flags=flags)
            return so, s, x_pool, adj_pool, self._rows_staged_loss(s, ptr, max_nodes)
        out = K.pool_rows_forward(x, weight, bias, s, *args)
        if out is None:  # kernels.pool_rows, with Select in front of the composed operators where it has not run yet
            if s is None:  # (not the one-call entry's case after all: the selector runs on its own, as the module has it)
                so, s = self._rows_select(x, batch, batched_out)
            out = K.pool_rows_forward_composed(x, None, None, s, *args)
        return so, out["s"], out["x_pool"], out["adj_pool"], out["both"] if mode == 1 else out["lossv"]

    def _rows_hand_out(self, sel, so, s_flat, x_pool, adj_pool, both_or_loss, mode, batch, batched_out, info, nb, max_nodes):
        """The route's ``_Pooled``: S as the mode hands it out, the loss dict, the pooled batch vector."""
        if batched_out:  # S as the batched mode hands it out: padded [B,Nmax,K] + the node mask (differentiable view of S)
            if s_flat.size(0) == nb * max_nodes:  # graphs of one size: the padded form is a view, the mask a constant
                s_pad = s_flat.view(nb, max_nodes, s_flat.size(1))
                mask = torch.ones(nb, max_nodes, dtype=torch.bool, device=s_flat.device)  # (a tensor of the caller's own)
            else:
                from ..src import to_dense_batch
                s_pad, mask = to_dense_batch(s_flat, batch, max_nodes, nb)
            so = SelectOutput(s=s_pad, s_inv_op=sel.s_inv_op, in_mask=mask)
            if info is not None:
                so._graph_sizes = info.sizes
        elif so is None:
            so = SelectOutput(s=s_flat, s_inv_op=sel.s_inv_op, batch=batch)
        loss = both_or_loss if mode == 0 else self._pair_loss(both_or_loss)
        batch_pool = self.reducer.reduce_batch(so, batch if batch is not None else so.batch)
        return _Pooled(so, x_pool, None, adj_pool, batch_pool=batch_pool, loss=loss)

    def _sizes_for(self, adj):
        """Real nodes per graph of the zero-padded batch ``adj`` belongs to, if forward() densified it itself."""
        # (_sizes_hint stays on the module, unlike the per-call node count: the public compute_loss reads it with no
        #  forward() in between, and it answers only for the very adjacency tensor it was noted for)
        hint = getattr(self, "_sizes_hint", None)
        return hint[1] if hint is not None and hint[0]() is adj else None

    @staticmethod
    def _real_nodes(known_nodes, mask):
        """Valid nodes of the padded batch: the host-side count when forward() had one, else a 0-dim device tensor
        (no host round trip either way)."""
        return known_nodes if known_nodes is not None else mask.sum()

    def _batched_output(self, x_pool, adj_pool, so, loss, batch, batch_pool) -> PoolingOutput:
        if self.sparse_output:
            x_pool, ei, ew, batch_pool = self._finalize_sparse_output(
                x_pool=x_pool, adj_pool=adj_pool, batch=batch, batch_pooled=batch_pool, so=so)
            return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so, loss=loss)
        return PoolingOutput(x=x_pool, edge_index=adj_pool, so=so, loss=loss)

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None,
                so: Optional[SelectOutput] = None, mask: Optional[Tensor] = None,
                batch: Optional[Tensor] = None, batch_pooled: Optional[Tensor] = None, lifting: bool = False,
                **kwargs):
        if lifting:
            return self._lift(x, so, batch, batch_pooled)
        if self.batched:
            if so is None and mask is None and not is_dense_adj(adj):
                self._sizes_hint = None
                # straight from the un-padded batch, no densification launches: small graphs in the one-launch kernel,
                # large sparse ones on the un-padded rows route (r6)
                pooled = self._select_reduce_connect_sparse(x, adj, edge_weight, batch)
                if pooled is None:
                    pooled = self._unbatched_fused(x, adj, edge_weight, batch, batched_out=True)
                if pooled is not None:
                    return self._batched_output(pooled.x_pool, pooled.adj_pool, pooled.so, pooled.loss, batch,
                                                pooled.batch_pool)
            # number of real nodes behind the padded batch, when the host already knows it (a reduction over the mask
            # costs ~25 us on the device for any mask size)
            known_nodes = None
            graph_sizes = None
            sparse_in = False
            if not is_dense_adj(adj) and isinstance(x, Tensor) and x.dim() == 2:
                sparse_in = True
                known_nodes = x.size(0)
                if batch is not None and batch.numel() > 0 and x.is_cuda:
                    graph_sizes = batch_info(batch).sizes  # memoised: the densification below asks for it anyway
            elif mask is None and isinstance(x, Tensor) and x.dim() == 3:
                known_nodes = x.size(0) * x.size(1)
            sparse_edges = (adj, edge_weight) if sparse_in else None
            adj_handed = is_dense_adj(adj)  # (a dense adjacency of the caller's: it may get a gradient on the fused routes)
            x, adj, mask = self._ensure_batched_inputs(x=x, edge_index=adj, edge_weight=edge_weight, batch=batch,
                                                       mask=mask)
            # (the folded kernels also write the pooled batch vector: arange(B).repeat_interleave(K) of the B graphs)
            want_bp = sparse_in and batch is not None and batch.dtype == torch.long and batch.numel() > 0
            pooled = self._select_reduce_connect(x, adj, mask, want_bp, known_nodes)
            if pooled is None and _FOLD_TRAINING:
                pooled = self._select_reduce_connect_train(x, adj, mask, graph_sizes, want_bp, known_nodes, adj_handed)
            symmetry = None
            if sparse_in and _FOLD_TRAINING and torch.is_grad_enabled() and isinstance(adj, Tensor) and adj.dim() == 3:
                # (asked only when the one-node path takes the call: a launch over the entries, answered in its backward)
                dense_adj, ei_in, ew_in = adj, sparse_edges[0], sparse_edges[1]
                symmetry = lambda: self._adj_symmetry(ei_in, ew_in, dense_adj, batch)  # noqa: E731
            elif (not sparse_in and _FOLD_TRAINING and torch.is_grad_enabled() and isinstance(adj, Tensor)
                  and adj.dim() == 3 and adj.is_contiguous() and not adj.requires_grad):
                # a dense adjacency the caller holds (e.g. one fixed graph pooled every epoch): one pass over it, once
                # per tensor object, tells whether A = A^T (the backward then forms one N^2 K product less).  Not for one
                # that requires a gradient: an activation is a fresh tensor every step, the memo would never hit and
                # cost a pass per step -- the general backward is taken
                held = adj
                symmetry = lambda: K.AdjSymmetry.of_dense(held)  # noqa: E731
            if pooled is None and _FOLD_TRAINING:  # graphs beyond the one-wave kernels: one autograd node as well (r6)
                pooled = self._select_reduce_connect_large(x, adj, mask, graph_sizes, symmetry=symmetry,
                                                           known_nodes=known_nodes, adj_handed=adj_handed)
            so = pooled.so if pooled is not None else self.select(x=x, mask=mask)
            self._sizes_hint = None
            if graph_sizes is not None and graph_sizes.numel() == x.size(0):
                so._graph_sizes = graph_sizes
                self._sizes_hint = (weakref.ref(adj), graph_sizes)  # valid for exactly this adjacency tensor
            if pooled is None:  # Reduce + Connect in one native call (training: batches of small graphs only)
                pooled = self._reduce_connect_pooled(x, adj, so, self._wants_raw, self._mincut_terms,
                                                     self._fused_diff_scales(adj, known_nodes),
                                                     adj_grad=(not self._loss_only
                                                               and self._adj_grad_ok(adj, self.connector, adj_handed)))
                if pooled is None and _FOLD_TRAINING:  # a selector with hidden layers made S: the pooling step is one node still
                    pooled = self._select_reduce_connect_large(x, adj, mask, graph_sizes, so=so, symmetry=symmetry,
                                                               known_nodes=known_nodes, adj_handed=adj_handed)
            if pooled is not None:
                x_pool, adj_pool, batch_pool = pooled.x_pool, pooled.adj_pool, pooled.batch_pool
                if batch_pool is None:
                    batch_pool = self.reducer.reduce_batch(so, batch if batch is not None else so.batch)
                loss = self._loss_from_fused(adj, so, mask, pooled.raw, pooled.terms, pooled.diff, known_nodes)
            else:
                x_pool, batch_pool = self.reduce(x=x, so=so, batch=batch)
                adj_pool, loss = self._batched_connect_and_loss(x, adj, so, mask, edge_weight, batch, batch_pool,
                                                                known_nodes)
            return self._batched_output(x_pool, adj_pool, so, loss, batch, batch_pool)
        # unbatched: S [N,K], sparse A, sparse losses
        pooled = self._unbatched_fused(x, adj, edge_weight, batch)
        if pooled is not None and pooled.x_pool is not None:  # the losses from the products the Connect forms anyway (r6)
            return PoolingOutput(x=pooled.x_pool, edge_index=pooled.adj_pool, edge_weight=None, batch=pooled.batch_pool,
                                 so=pooled.so, loss=pooled.loss)
        so = pooled.so if pooled is not None else self.select(x=x, batch=batch)
        loss = self._sparse_loss(adj, edge_weight, so.s, batch)
        x_pool, batch_pool = self.reduce(x=x, so=so, batch=batch, return_batched=not self.sparse_output)
        ei, ew = self.connect(edge_index=adj, so=so, edge_weight=edge_weight, batch=batch,
                              batch_pooled=batch_pool)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so, loss=loss)


class DiffPool(_DenseMLPPooling):
    r"""DiffPool: S = softmax(MLP(X)), X' = S^T X, A' = S^T A S, link-prediction + entropy auxiliary
    losses (reference poolers/diffpool.py:22-331)."""

    def __init__(self, in_channels: Union[int, List[int]], k: int, act: str = None, dropout: float = 0.0,
                 link_loss_coeff: float = 1.0, ent_loss_coeff: float = 1.0, normalize_loss: bool = False,
                 remove_self_loops: bool = True, degree_norm: bool = True, edge_weight_norm: bool = False,
                 adj_transpose: bool = True, lift: str = "precomputed", s_inv_op: str = "transpose",
                 batched: bool = True, sparse_output: bool = False, cache_preprocessing: bool = False):
        super().__init__(in_channels, k, act, dropout, remove_self_loops, degree_norm, edge_weight_norm,
                         adj_transpose, lift, s_inv_op, batched, sparse_output, cache_preprocessing)
        self.link_loss_coeff = link_loss_coeff
        self.ent_loss_coeff = ent_loss_coeff
        self.normalize_loss = normalize_loss

    _connects_through_operator = True
    _sparse_diff_stats = True
    _rows_mode = 2

    def _loss_scales(self, adj_numel, num_nodes):
        """(link_scale, ent_scale): the coefficients with the two normalisations folded in (``adj_numel``: adj.numel()
        of the padded batch, losses.py:651, or a callable asked only when the link loss is normalised)."""
        link_scale = self.link_loss_coeff
        if self.normalize_loss is True:
            link_scale = link_scale / (adj_numel() if callable(adj_numel) else adj_numel)
        return (float(link_scale), float(self.ent_loss_coeff) / num_nodes)

    def _fused_diff_scales(self, adj, known_nodes, adj_numel=None):
        if not (isinstance(known_nodes, int) and known_nodes > 0):
            return None
        return self._loss_scales(adj.numel() if adj_numel is None else adj_numel, known_nodes)

    def _sparse_launch_loss(self, s, mask, raw, terms, stats, edges, info, num_nodes) -> dict:
        # inference (r6): both losses from per-graph records of the same launch -- no dense adjacency
        scales = self._loss_scales(info.num_graphs * info.max_nodes * info.max_nodes, num_nodes)
        return self._pair_loss(K.diffpool_stats_tail(stats, scales[0], scales[1]))

    def _pair_loss(self, both) -> dict:
        return {"link_loss": both[0], "entropy_loss": both[1]}

    def _loss_from_fused(self, adj, so, mask, raw, terms=None, diff=None, known_nodes=None) -> dict:
        if diff is not None:  # both losses came with the fused call (and are differentiated by its backward)
            return self._pair_loss(diff)
        return self.compute_loss(adj=adj, S=so.s, num_nodes=self._real_nodes(known_nodes, mask))

    def compute_loss(self, adj: Tensor, S: Tensor, num_nodes: int) -> dict:
        if (S.is_cuda and S.dim() == 3 and S.dtype == torch.float32 and adj.dim() == 3 and adj.is_contiguous()
                and isinstance(num_nodes, int) and num_nodes > 0
                and not (torch.is_grad_enabled() and (S.requires_grad or adj.requires_grad))):
            # inference: both losses from their native partial reductions and one tail launch (as torch ops behind
            # the kernels: sum, sqrt, a final-sum kernel, a division and two multiplications)
            link_scale, ent_scale = self._loss_scales(adj.numel(), num_nodes)
            return self._pair_loss(K.diffpool_loss_tail(S, adj, self._sizes_for(adj), link_scale, ent_scale))
        return {"link_loss": link_pred_loss(S, adj, normalize_loss=self.normalize_loss,
                                            graph_sizes=self._sizes_for(adj)) * self.link_loss_coeff,
                "entropy_loss": entropy_loss(S, num_nodes) * self.ent_loss_coeff}

    def compute_sparse_loss(self, edge_index, edge_weight, S, batch) -> dict:
        ei, ew = connectivity_to_edge_index(edge_index, edge_weight)
        return {"link_loss": sparse_link_pred_loss(S, ei, ew, batch, normalize_loss=self.normalize_loss)
                * self.link_loss_coeff,
                "entropy_loss": unbatched_entropy_loss(S) * self.ent_loss_coeff}

    def extra_repr_args(self) -> dict:
        return {"batched": self.batched, "link_loss_coeff": self.link_loss_coeff,
                "ent_loss_coeff": self.ent_loss_coeff, "normalize_loss": self.normalize_loss}


class MinCutPooling(_DenseMLPPooling):
    r"""MinCut pooling: as DiffPool, with the normalised-cut and orthogonality losses computed on the
    *raw* S^T A S before it is post-processed (reference poolers/mincut.py:22-354)."""

    def __init__(self, in_channels: Union[int, List[int]], k: int, act: str = None, dropout: float = 0.0,
                 cut_loss_coeff: float = 1.0, ortho_loss_coeff: float = 1.0, remove_self_loops: bool = True,
                 degree_norm: bool = True, edge_weight_norm: bool = False, adj_transpose: bool = True,
                 lift: str = "precomputed", s_inv_op: str = "transpose", batched: bool = True,
                 sparse_output: bool = False, cache_preprocessing: bool = False):
        super().__init__(in_channels, k, act, dropout, remove_self_loops, degree_norm, edge_weight_norm,
                         adj_transpose, lift, s_inv_op, batched, sparse_output, cache_preprocessing)
        self.cut_loss_coeff = cut_loss_coeff
        self.ortho_loss_coeff = ortho_loss_coeff

    def _lift(self, x, so, batch, batch_pooled):
        return self.lift(x_pool=x, so=so, batch=batch if batch is not None else so.batch,
                         batch_pooled=batch_pooled)

    _loss_kind = "mincut"
    _rows_mode = 1

    def _pair_loss(self, both) -> dict:
        return {"cut_loss": both[0] if self.cut_loss_coeff == 1 else both[0] * self.cut_loss_coeff,
                "ortho_loss": both[1] if self.ortho_loss_coeff == 1 else both[1] * self.ortho_loss_coeff}

    def _sparse_launch_loss(self, s, mask, raw, terms, stats, edges, info, num_nodes) -> dict:
        return self._pair_loss(terms.mean(dim=1))

    def _loss_from_fused(self, adj, so, mask, raw, terms=None, diff=None, known_nodes=None) -> dict:
        if terms is not None and so.s.dtype == torch.float32:
            # both per-graph loss tails came out of the pooling kernel itself (batches of small graphs); under autograd
            # their batch means arrive as two 0-dim outputs of the fused Function (functions.LossPair)
            return self._pair_loss(terms if isinstance(terms, LossPair) else terms.mean(dim=1))
        return self.compute_loss(adj, so.s, raw)

    def compute_loss(self, adj: Tensor, S: Tensor, adj_pooled: Tensor) -> dict:
        if (S.is_cuda and S.dim() == 3 and S.dtype == torch.float32
                and not (torch.is_grad_enabled() and (S.requires_grad or adj.requires_grad
                                                       or adj_pooled.requires_grad))):
            # inference: both losses' per-graph tails in one launch (as torch ops: ~14 launches of a few hundred bytes)
            return self._pair_loss(mincut_loss_terms(adj, S, adj_pooled, graph_sizes=self._sizes_for(adj)).mean(dim=1))
        if (S.is_cuda and S.dim() == 3 and S.dtype == torch.float32 and adj.dim() == 3 and not adj.requires_grad
                and adj_pooled.dtype == torch.float32 and adj_pooled.dim() == 3):
            # training: both losses as one Function with a native backward tail (the adjacency gets no gradient there)
            return self._pair_loss(_MinCutTermsFn.apply(adj, S, adj_pooled, self._sizes_for(adj)).mean(dim=1))
        return {"cut_loss": mincut_loss(adj, S, adj_pooled, batch_reduction="mean",
                                        graph_sizes=self._sizes_for(adj)) * self.cut_loss_coeff,
                "ortho_loss": orthogonality_loss(S, batch_reduction="mean",
                                                 graph_sizes=self._sizes_for(adj)) * self.ortho_loss_coeff}

    def compute_sparse_loss(self, edge_index, edge_weight, S, batch) -> dict:
        ei, ew = connectivity_to_edge_index(edge_index, edge_weight)
        return {"cut_loss": sparse_mincut_loss(ei, S, ew, batch, batch_reduction="mean") * self.cut_loss_coeff,
                "ortho_loss": unbatched_orthogonality_loss(S, batch, batch_reduction="mean")
                * self.ortho_loss_coeff}

    def extra_repr_args(self) -> dict:
        return {"batched": self.batched, "cut_loss_coeff": self.cut_loss_coeff,
                "ortho_loss_coeff": self.ortho_loss_coeff}


class DMoNPooling(_DenseMLPPooling):
    r"""DMoN pooling: MinCut's Select / Reduce / Connect with the spectral (modularity), cluster and orthogonality losses
    on the *raw* S^T A S (reference poolers/dmon.py:23-333).  Batched: the losses read the densified adjacency (A^T when
    ``adj_transpose``: in-degrees), padded nodes excluded by the mask; unbatched: out-degrees of the edge list."""

    _loss_kind = "dmon"

    def __init__(self, in_channels: Union[int, List[int]], k: int, act: str = None, dropout: float = 0.0,
                 spectral_loss_coeff: float = 1.0, cluster_loss_coeff: float = 1.0, ortho_loss_coeff: float = 0.0,
                 remove_self_loops: bool = True, degree_norm: bool = True, edge_weight_norm: bool = False,
                 adj_transpose: bool = True, lift: str = "precomputed", s_inv_op: str = "transpose",
                 batched: bool = True, sparse_output: bool = False, cache_preprocessing: bool = False):
        super().__init__(in_channels, k, act, dropout, remove_self_loops, degree_norm, edge_weight_norm,
                         adj_transpose, lift, s_inv_op, batched, sparse_output, cache_preprocessing)
        self.spectral_loss_coeff = spectral_loss_coeff
        self.ortho_loss_coeff = ortho_loss_coeff
        self.cluster_loss_coeff = cluster_loss_coeff

    def _sparse_launch_loss(self, s, mask, raw, terms, stats, edges, info, num_nodes) -> dict:
        # raw from the launch, degrees from the edge list: no dense adjacency either
        edge_index, edge_weight, edge_ptr = edges
        deg = K.dmon_edge_degrees(edge_index, edge_weight, info.ptr, edge_ptr, info.max_nodes, self.adj_transpose)
        return self._dmon_means(s, raw, mask, info.sizes, deg=deg)

    def _loss_from_fused(self, adj, so, mask, raw, terms=None, diff=None, known_nodes=None) -> dict:
        return self.compute_loss(adj, so.s, raw, mask)

    def _dmon_means(self, S, raw, mask, graph_sizes, adj=None, deg=None) -> dict:
        """The batch means of the three terms (coefficients applied) from one pass over adj or the given degrees, one
        over S, S^T S and one tail launch."""
        coeffs = (self.spectral_loss_coeff, self.cluster_loss_coeff, self.ortho_loss_coeff)
        three = dmon_loss_terms(adj, S, raw, mask, graph_sizes, coeffs, deg=deg).mean(dim=1)
        return {"spectral_loss": three[0], "cluster_loss": three[1], "ortho_loss": three[2]}

    def _scaled(self, spectral, cluster, ortho) -> dict:
        return {"spectral_loss": spectral if self.spectral_loss_coeff == 1 else spectral * self.spectral_loss_coeff,
                "cluster_loss": cluster if self.cluster_loss_coeff == 1 else cluster * self.cluster_loss_coeff,
                "ortho_loss": ortho if self.ortho_loss_coeff == 1 else ortho * self.ortho_loss_coeff}

    def compute_loss(self, adj: Tensor, S: Tensor, adj_pooled: Tensor, mask: Optional[Tensor]) -> dict:
        if (_native_f32(adj, S, adj_pooled) and S.dim() == 3 and adj.dim() == 3 and adj_pooled.dim() == 3
                and not adj.requires_grad):
            # the three per-graph tails from one pass over adj, one over S, S^T S and one tail launch (native backward)
            return self._dmon_means(S, adj_pooled, mask, self._sizes_for(adj), adj=adj)
        return self._scaled(spectral_loss(adj, S, adj_pooled, mask, batch_reduction="mean"),
                            cluster_loss(S, mask=mask, batch_reduction="mean"),
                            orthogonality_loss(S, batch_reduction="mean"))

    def compute_sparse_loss(self, edge_index, edge_weight, S, batch) -> dict:
        ei, ew = connectivity_to_edge_index(edge_index, edge_weight)
        return self._scaled(sparse_spectral_loss(ei, S, ew, batch, batch_reduction="mean"),
                            unbatched_cluster_loss(S, batch, batch_reduction="mean"),
                            unbatched_orthogonality_loss(S, batch, batch_reduction="mean"))

    def extra_repr_args(self) -> dict:
        return {"batched": self.batched, "spectral_loss_coeff": self.spectral_loss_coeff,
                "cluster_loss_coeff": self.cluster_loss_coeff, "ortho_loss_coeff": self.ortho_loss_coeff}


class JustBalancePooling(_DenseMLPPooling):
    r"""Just Balance pooling ("Simplifying Clustering with Graph Neural Networks", Bianchi, NLDL 2023; reference
    poolers/just_balance.py:17-322): MinCut's Select / Reduce / Connect with the single balance loss
    -trace(sqrt(S^T S + eps)), by default divided by sqrt(n K) per graph, times ``loss_coeff``.  The loss reads S alone
    -- neither the adjacency nor S^T A S -- and only the diagonal of S^T S is ever computed.

    A NaN loss raises ``ValueError("Loss is NaN")`` where the loss is composed of torch ops (float64, host tensors, an
    unsorted batch vector); behind the loss kernel the check would be a wait for the device and is not made.
    ``data_transforms()`` returns None: the reference's ``NormalizeAdj`` lives in its ``tgp.data``, which this project
    does not have."""

    _loss_kind = "jb"

    def __init__(self, in_channels: Union[int, List[int]], k: int, act: str = None, dropout: float = 0.0,
                 normalize_loss: bool = True, loss_coeff: float = 1.0, remove_self_loops: bool = True,
                 degree_norm: bool = True, edge_weight_norm: bool = False, adj_transpose: bool = True,
                 lift: str = "precomputed", s_inv_op: str = "transpose", batched: bool = True,
                 sparse_output: bool = False, cache_preprocessing: bool = False):
        super().__init__(in_channels, k, act, dropout, remove_self_loops, degree_norm, edge_weight_norm,
                         adj_transpose, lift, s_inv_op, batched, sparse_output, cache_preprocessing)
        self.normalize_loss = normalize_loss
        self.loss_coeff = loss_coeff

    _connects_through_operator = True
    _rows_mode = 0

    def _sparse_launch_loss(self, s, mask, raw, terms, stats, edges, info, num_nodes) -> dict:
        # the launch writes S; the loss reads nothing else: no dense adjacency, no raw
        return self._jb_mean(s, mask, info.sizes)

    def _rows_staged_loss(self, s, ptr, max_nodes) -> dict:
        return {"balance_loss": K.jb_terms(s, ptr=ptr, max_nodes=max_nodes, normalize=bool(self.normalize_loss),
                                           scale=float(self.loss_coeff), want_coef=False, want_mean=True)[2]}

    def _loss_from_fused(self, adj, so, mask, raw, terms=None, diff=None, known_nodes=None) -> dict:
        graph_sizes = self._sizes_for(adj)
        if graph_sizes is not None and _jb_native(so.s):
            # (the selector zeroed the padded rows of its own S, so the pass over S stops at each graph's size)
            return self._jb_mean(so.s, mask, graph_sizes)
        return self.compute_loss(so.s, mask, so.num_nodes, so.num_supernodes)

    def _jb_mean(self, S, mask, graph_sizes) -> dict:
        """The batch mean of the per-graph loss, ``loss_coeff`` applied by the loss kernel itself."""
        return {"balance_loss": jb_loss_mean(S, mask, graph_sizes, None, self.normalize_loss, scale=self.loss_coeff)}

    def compute_loss(self, S: Tensor, mask: Optional[Tensor] = None, num_nodes: Optional[int] = None,
                     num_supernodes: Optional[int] = None) -> dict:
        loss = jb_loss_mean(S, mask, None, None, self.normalize_loss, num_nodes, num_supernodes, scale=self.loss_coeff)
        if not _jb_native(S) and torch.isnan(loss):  # (behind the kernel the check would be a wait for the device)
            raise ValueError("Loss is NaN")
        return {"balance_loss": loss}

    def compute_sparse_loss(self, S: Tensor, batch: Optional[Tensor]) -> dict:
        loss = jb_loss_mean(S, batch=batch, normalize_loss=self.normalize_loss, scale=self.loss_coeff)
        if not _jb_native(S, batch) and torch.isnan(loss):
            raise ValueError("Loss is NaN")
        return {"balance_loss": loss}

    def _sparse_loss(self, edge_index, edge_weight, S, batch) -> dict:
        return self.compute_sparse_loss(S, batch)

    @staticmethod
    def data_transforms():
        return None

    def extra_repr_args(self) -> dict:
        return {"batched": self.batched, "loss_coeff": self.loss_coeff, "normalize_loss": self.normalize_loss}


class AsymCheegerCutPooling(_DenseMLPPooling):
    r"""Asymmetric Cheeger cut pooling ("Total Variation Graph Neural Networks", Hansen & Bianchi, ICML 2023; reference
    poolers/asym_cheeger_cut.py:22-321): MinCut's Select / Reduce / Connect with the total-variation loss
    sum_ij a_ij ||s_i - s_j||_1 / (2 E) and the balance (asymmetric norm) loss around each column's quantile.  Batched:
    the losses read the densified adjacency (its nonzero entries are the edges) and the mask; unbatched: the edge list
    (every edge counts, zero-weight ones included).

    Ties: where several nodes of a graph hold a column's quantile value, the quantile's gradient goes to the LOWEST node
    index among them (the reference sorts unstably and leaves that open)."""

    _loss_kind = "acc"

    def __init__(self, in_channels: Union[int, List[int]], k: int, act: str = None, dropout: float = 0.0,
                 totvar_coeff: float = 1.0, balance_coeff: float = 1.0, remove_self_loops: bool = True,
                 degree_norm: bool = True, edge_weight_norm: bool = False, adj_transpose: bool = True,
                 lift: str = "precomputed", s_inv_op: str = "transpose", batched: bool = True,
                 sparse_output: bool = False, cache_preprocessing: bool = False):
        super().__init__(in_channels, k, act, dropout, remove_self_loops, degree_norm, edge_weight_norm,
                         adj_transpose, lift, s_inv_op, batched, sparse_output, cache_preprocessing)
        self.k = k
        self.totvar_coeff = totvar_coeff
        self.balance_coeff = balance_coeff

    def _loss_from_fused(self, adj, so, mask, raw, terms=None, diff=None, known_nodes=None) -> dict:
        return self.compute_loss(adj, so.s, mask)

    def _scaled(self, tv, bal) -> dict:
        return {"total_variation_loss": tv if self.totvar_coeff == 1 else tv * self.totvar_coeff,
                "balance_loss": bal if self.balance_coeff == 1 else bal * self.balance_coeff}

    def compute_loss(self, adj: Tensor, S: Tensor, mask: Optional[Tensor] = None) -> dict:
        if _native_f32(adj, S) and S.dim() == 3 and adj.dim() == 3 and not adj.requires_grad:
            # both per-graph terms, coefficients applied: the pass over adj's nonzeros, the quantile select, one tail
            # launch (native backward)
            both = acc_loss_terms(adj, S, self.k, mask, self._sizes_for(adj),
                                  (self.totvar_coeff, self.balance_coeff)).mean(dim=1)
            return {"total_variation_loss": both[0], "balance_loss": both[1]}
        return self._scaled(totvar_loss(S, adj, batch_reduction="mean"),
                            asym_norm_loss(S, self.k, mask=mask, batch_reduction="mean"))

    def compute_sparse_loss(self, edge_index, edge_weight, S, batch) -> dict:
        ei, ew = connectivity_to_edge_index(edge_index, edge_weight)
        both = acc_sparse_loss_terms(ei, ew, S, self.k, batch, (self.totvar_coeff, self.balance_coeff))
        if both is not None:  # one Function, one tail launch, coefficients applied (as the dense route)
            both = both.mean(dim=1)
            return {"total_variation_loss": both[0], "balance_loss": both[1]}
        return self._scaled(sparse_totvar_loss(ei, S, ew, batch, batch_reduction="mean"),
                            unbatched_asym_norm_loss(S, self.k, batch, batch_reduction="mean"))

    def extra_repr_args(self) -> dict:
        return {"batched": self.batched, "totvar_coeff": self.totvar_coeff, "balance_coeff": self.balance_coeff}


class HOSCPooling(_DenseMLPPooling):
    r"""Higher-order spectral clustering pooling ("Higher-order clustering and pooling for Graph Neural Networks", Duval &
    Malliaros, CIKM 2022; reference poolers/hosc.py:25-384): MinCut's Select / Reduce / Connect with the loss
    ``hosc_loss`` = ((1 - alpha) cut + alpha ho_cut) / k -- cut MinCut's first-order cut on the raw S^T A S, ho_cut the
    same cut of the motif adjacency M = A A A -- and ``ortho_loss`` = mu x MinCut's orthogonality term or, with
    ``hosc_ortho``, mu (sqrt(K) - sum_j ||S_*j|| / sqrt(n)) / (sqrt(K) - 1).

    M is never formed: trace(S^T M S) = sum S (.) A (A (A S)) and M 1 = A (A (A 1)) (the reference's batched mode
    multiplies A A A out; its unbatched function already uses the chain).  Batched: the losses read the densified
    adjacency (A^T when ``adj_transpose``: in-degrees); unbatched: the edge list (out-degrees), so the two modes
    disagree on a directed graph, as in the reference.  A disabled term (``mu = 0``, ``K <= 1``) is a float32 0-dim zero
    on the inputs' device, where the reference hands out an int64 host zero."""

    _loss_kind = "hosc"

    def __init__(self, in_channels: Union[int, List[int]], k: int, act: str = None, dropout: float = 0.0,
                 mu: float = 0.1, alpha: float = 0.5, hosc_ortho: bool = False, remove_self_loops: bool = True,
                 degree_norm: bool = True, edge_weight_norm: bool = False, adj_transpose: bool = True,
                 lift: str = "precomputed", s_inv_op: str = "transpose", batched: bool = True,
                 sparse_output: bool = False, cache_preprocessing: bool = False):
        super().__init__(in_channels, k, act, dropout, remove_self_loops, degree_norm, edge_weight_norm,
                         adj_transpose, lift, s_inv_op, batched, sparse_output, cache_preprocessing)
        self.k = k
        self.mu = mu
        self.alpha = alpha
        self.hosc_ortho = hosc_ortho

    def _loss_from_fused(self, adj, so, mask, raw, terms=None, diff=None, known_nodes=None) -> dict:
        return self.compute_loss(adj, so.s, raw, mask)

    def compute_loss(self, adj: Tensor, S: Tensor, adj_pool: Tensor, mask: Optional[Tensor] = None) -> dict:
        if (_native_f32(adj, S, adj_pool) and S.dim() == 3 and adj.dim() == 3 and adj_pool.dim() == 3
                and not adj.requires_grad):
            # both per-graph rows, alpha, mu and 1 / k applied: the motif chain, one pass over S, one tail launch
            both = hosc_loss_terms(adj, S, adj_pool, mask, self._sizes_for(adj), self.alpha, self.mu, self.k,
                                   self.hosc_ortho).mean(dim=1)
            return {"hosc_loss": both[0], "ortho_loss": both[1]}
        cut = ho_cut = 0.0
        if self.alpha < 1:
            cut = mincut_loss(adj, S, adj_pool, batch_reduction="mean") / self.k
        if self.alpha > 0:
            ho_cut = _ho_cut_composed_dense(adj, S).mean() / self.k
        if self.mu == 0:
            ortho = S.new_zeros(())
        elif self.hosc_ortho:
            # (the reference's pooler always holds a mask -- all true for dense inputs given without one -- and takes
            #  the square root of its integer row sums in float32)
            full = mask if mask is not None else torch.ones(S.shape[:2], dtype=torch.bool, device=S.device)
            ortho = hosc_orthogonality_loss(S, full, batch_reduction="mean")
        else:
            ortho = orthogonality_loss(S, batch_reduction="mean")
        return {"hosc_loss": (1 - self.alpha) * cut + self.alpha * ho_cut, "ortho_loss": self.mu * ortho}

    def compute_sparse_loss(self, edge_index, edge_weight, S, batch) -> dict:
        ei, ew = connectivity_to_edge_index(edge_index, edge_weight)
        both = hosc_sparse_loss_terms(ei, ew, S, batch, self.alpha, self.mu, self.k, self.hosc_ortho)
        if both is not None:  # one Function, one tail launch, alpha, mu and 1 / k applied (as the dense route)
            both = both.mean(dim=1)
            return {"hosc_loss": both[0], "ortho_loss": both[1]}
        cut = ho_cut = S.new_zeros(())
        if self.alpha < 1:
            cut = sparse_mincut_loss(ei, S, ew, batch, batch_reduction="mean") / self.k
        if self.alpha > 0:
            ho_cut = sparse_ho_mincut_loss(ei, S, ew, batch, batch_reduction="mean") / self.k
        if self.mu == 0:
            ortho = S.new_zeros(())
        elif self.hosc_ortho:
            ortho = unbatched_hosc_orthogonality_loss(S, batch, batch_reduction="mean")
        else:
            ortho = unbatched_orthogonality_loss(S, batch, batch_reduction="mean")
        return {"hosc_loss": (1 - self.alpha) * cut + self.alpha * ho_cut, "ortho_loss": self.mu * ortho}

    def extra_repr_args(self) -> dict:
        return {"batched": self.batched, "mu": self.mu, "alpha": self.alpha, "hosc_ortho": self.hosc_ortho}


class BNPool(_DenseMLPPooling):
    r"""BN-Pool ("BN-Pool: Bayesian Nonparametric Graph Pooling", Castellana & Bianchi 2025; reference
    poolers/bnpool.py:27-556): the assignment comes from a truncated stick-breaking process (:class:`~tgp.select.DPSelect`),
    Reduce and Connect are MinCut's, and three losses train it: ``quality``, the class-balanced binary cross entropy between
    the logits S K S^T and the adjacency divided by n^2 (K a learnable k x k matrix); ``kl`` = eta x the KL divergence of
    the sticks' Beta posteriors from the Beta(1, alpha_DP) prior; ``K_prior``, a Gaussian prior on K.

    Batched: the reconstruction loss reads the preprocessed dense adjacency (A^T when ``adj_transpose``) and the mask;
    float32 device tensors take the native route (utils.losses.bnpool_rec_loss_terms: the [B,N,N] logits are never
    formed, forward or backward), float64 the composed one.  Unbatched: the reference's sampled-edge loss over the edge
    list and the pairs :meth:`sample_negative_edges` draws (the project's own sampler, utils.ops); the per-graph
    sampled-edge count normalises ``kl`` and ``K_prior``.

    With ``train_K=False`` ``K_prior`` is a float32 0-dim zero on the inputs' device (the reference hands out a host
    tensor)."""

    _loss_kind = "bnpool"

    def __init__(self, in_channels: Union[int, List[int]], k: int, alpha_DP=1.0, K_var=1.0, K_mu=10.0, K_init=1.0,
                 eta=1.0, train_K=True, act: str = None, dropout: float = 0.0, remove_self_loops: bool = True,
                 degree_norm: bool = True, edge_weight_norm: bool = False, adj_transpose: bool = True,
                 lift: str = "precomputed", s_inv_op: str = "transpose", batched: bool = True,
                 sparse_output: bool = False, cache_preprocessing: bool = False,
                 num_neg_samples: Optional[int] = None):
        if alpha_DP <= 0:
            raise ValueError("alpha_DP must be positive")
        if K_var <= 0:
            raise ValueError("K_var must be positive")
        if eta <= 0:
            raise ValueError("eta must be positive")
        if k <= 0:
            raise ValueError("max_k must be positive")
        super().__init__(in_channels, k, act, dropout, remove_self_loops, degree_norm, edge_weight_norm,
                         adj_transpose, lift, s_inv_op, batched, sparse_output, cache_preprocessing)
        self.selector = DPSelect(in_channels, k, batched_representation=batched, act=act, dropout=dropout,
                                 s_inv_op=s_inv_op)
        self.k = k
        self.K_init_val = K_init
        self.alpha_DP = alpha_DP
        self.K_var_val = K_var
        self.K_mu_val = K_mu
        self.train_K = train_K
        self.eta = eta
        self.num_neg_samples = num_neg_samples
        # prior of the stick-breaking process, prior of the cluster-cluster matrix, the matrix itself
        self.register_buffer("alpha_prior", torch.ones(self.k - 1))
        self.register_buffer("beta_prior", torch.ones(self.k - 1) * alpha_DP)
        self.register_buffer("K_var", torch.tensor(K_var))
        eye = torch.eye(self.k, self.k)
        self.register_buffer("K_mu", K_mu * eye - K_mu * (1 - eye))
        self.K = torch.nn.Parameter(K_init * eye - K_init * (1 - eye), requires_grad=train_K)

    def reset_parameters(self):
        super().reset_parameters()
        eye = torch.eye(self.k, self.k, device=self.K.device)
        self.K.data = self.K_init_val * eye - self.K_init_val * (1 - eye)

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None, so: Optional[SelectOutput] = None,
                batch: Optional[Tensor] = None, batch_pooled: Optional[Tensor] = None, lifting: bool = False,
                mask: Optional[Tensor] = None, **kwargs):
        if lifting or self.batched:
            return super().forward(x, adj, edge_weight, so=so, mask=mask, batch=batch, batch_pooled=batch_pooled,
                                   lifting=lifting, **kwargs)
        # unbatched: S [N,K], the sampled-edge loss, sparse Reduce and Connect
        so = self.select(x=x, batch=batch)
        loss = self.compute_sparse_loss(adj, batch, so)
        x_pool, batch_pool = self.reduce(x=x, so=so, batch=batch, return_batched=not self.sparse_output)
        ei, ew = self.connect(edge_index=adj, so=so, edge_weight=edge_weight, batch=batch, batch_pooled=batch_pool)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so, loss=loss)

    _connects_through_operator = True

    def _loss_from_fused(self, adj, so, mask, raw, terms=None, diff=None, known_nodes=None) -> dict:
        return self.compute_loss(adj, mask, so)

    def _prior_terms(self, q_z, norm_const, like: Tensor, **where) -> dict:
        """``kl`` and ``K_prior`` (composed torch ops, element-wise over [.., k-1] and [k,k])."""
        prior = torch.distributions.Beta(self.get_buffer("alpha_prior"), self.get_buffer("beta_prior"))
        kl = kl_loss(q_z, prior, normalizing_const=norm_const, batch_reduction="mean", **where)
        if self.train_K:
            k_prior = cluster_connectivity_prior_loss(self.K, self.get_buffer("K_mu"), self.get_buffer("K_var"),
                                                      normalizing_const=norm_const, batch_reduction="mean")
        else:
            k_prior = torch.zeros((), dtype=torch.float32, device=like.device)
        return {"kl": self.eta * kl, "K_prior": k_prior}

    def compute_loss(self, adj: Tensor, mask: Optional[Tensor], so: SelectOutput) -> dict:
        s, q_z = so.s, so.q_z
        n = mask.sum(-1) if mask is not None else torch.tensor(adj.shape[-1], device=adj.device)
        n_squared = n ** 2
        if _native_f32(s, self.K, adj) and s.dim() == 3 and adj.dim() == 3 and not adj.requires_grad:
            # per-graph terms, already divided by n^2: T = S K, one launch over the logit tiles, one tail launch
            rec = bnpool_rec_loss_terms(s, self.K, adj, mask).mean()
        else:
            rec = weighted_bce_reconstruction_loss(self.get_rec_adj(s), adj, mask, balance_links=True,
                                                   normalizing_const=n_squared, batch_reduction="mean")
        out = {"quality": rec}
        out.update(self._prior_terms(q_z, n_squared, s, mask=mask))
        return out

    def sample_negative_edges(self, edge_index: Tensor, batch: Optional[Tensor]) -> Tensor:
        """The non-edges the unbatched loss scores next to the edge list: undirected pairs, at most ``num_neg_samples`` per
        graph (None: as many as the graph has edges)."""
        if batch is None:
            return negative_edge_sampling(edge_index, num_neg_samples=self.num_neg_samples, force_undirected=True)
        return batched_negative_edge_sampling(edge_index, batch, num_neg_samples=self.num_neg_samples,
                                              force_undirected=True)

    def get_sparse_rec_loss(self, node_assignment: Tensor, adj, batch: Optional[Tensor], batch_size: int):
        """(loss, sampled-edge count per graph) over the edge list and the sampled non-edges."""
        edge_index, _ = connectivity_to_edge_index(adj)
        neg_edge_index = self.sample_negative_edges(edge_index, batch)
        all_edges = torch.cat([edge_index, neg_edge_index], dim=1)
        logits = self.get_prob_link_logit(node_assignment, all_edges)
        y = torch.cat([logits.new_ones(edge_index.size(1)), logits.new_zeros(neg_edge_index.size(1))], dim=0)
        return sparse_bce_reconstruction_loss(logits, y, edges_batch_id=None if batch is None else batch[all_edges[0]],
                                              batch_size=batch_size)

    def compute_sparse_loss(self, adj, batch: Optional[Tensor], so: SelectOutput) -> dict:
        from ..utils.ops import num_graphs_of
        batch_size = num_graphs_of(batch) if batch is not None else 1
        rec, norm_const = self.get_sparse_rec_loss(so.s, adj, batch, batch_size)
        out = {"quality": rec}
        where = dict(batch=batch, batch_size=batch_size) if batch is not None else {}
        out.update(self._prior_terms(so.q_z, norm_const, so.s, **where))
        return out

    def get_rec_adj(self, S: Tensor) -> Tensor:
        """The reconstructed adjacency's logits S K S^T (composed route and inspection; the native loss never forms it)."""
        return S @ self.K @ S.transpose(-1, -2)

    def get_prob_link_logit(self, node_assignment: Tensor, edges_list: Tensor) -> Tensor:
        """Logits (S[u] K) . S[v] of the node pairs ``edges_list`` [2,E]."""
        return ((node_assignment[edges_list[0]] @ self.K) * node_assignment[edges_list[1]]).sum(-1)

    def extra_repr_args(self) -> dict:
        return {"batched": self.batched, "alpha_DP": self.alpha_DP, "k_prior_variance": self.K_var_val,
                "k_prior_mean": self.K_mu_val, "k_init_value": self.K_init_val, "eta": self.eta, "train_K": self.train_K,
                "num_neg_samples": self.num_neg_samples}


class LaPooling(DenseSRCPooling):
    r"""LaPool (Noutahi et al. 2019; reference poolers/lapool.py): :class:`~tgp.select.LaPoolSelect`,
    :class:`~tgp.reduce.BaseReduce`, :class:`~tgp.connect.DenseConnect`, :class:`~tgp.lift.BaseLift`.  No learned
    layer and no auxiliary loss.  Constructor arguments, defaults, the batched / unbatched control flow, the
    ``sparse_output`` finalisation and lifting follow the reference.

    Differences from the reference: ``shortest_path_reg=True`` raises ``NotImplementedError`` (scipy on the host there);
    the ``"lap"`` alias of ``get_pooler`` is not registered yet; see :class:`~tgp.select.LaPoolSelect` for the
    selector's."""

    def __init__(self, shortest_path_reg: bool = False, remove_self_loops: bool = True, degree_norm: bool = True,
                 edge_weight_norm: bool = False, lift: str = "precomputed", s_inv_op: str = "transpose",
                 lift_red_op: str = "sum", batched: bool = True, sparse_output: bool = False):
        super().__init__(
            selector=LaPoolSelect(shortest_path_reg=shortest_path_reg, batched_representation=batched,
                                  s_inv_op=s_inv_op),
            reducer=BaseReduce(),
            lifter=BaseLift(matrix_op=lift, reduce_op=lift_red_op),
            connector=DenseConnect(remove_self_loops=remove_self_loops, degree_norm=degree_norm,
                                   edge_weight_norm=edge_weight_norm, sparse_output=sparse_output),
            batched=batched, sparse_output=sparse_output)

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None,
                so: Optional[SelectOutput] = None, batch: Optional[Tensor] = None,
                batch_pooled: Optional[Tensor] = None, lifting: bool = False, mask: Optional[Tensor] = None,
                **kwargs):
        if lifting:
            return self.lift(x_pool=x, so=so, batch=batch if batch is not None else so.batch,
                             batch_pooled=batch_pooled)
        if self.batched:
            x, adj, mask = self._ensure_batched_inputs(x=x, edge_index=adj, edge_weight=edge_weight, batch=batch,
                                                       mask=mask)
            so = self.select(x=x, edge_index=adj, mask=mask)
            x_pool, batch_pooled = self.reduce(x=x, so=so, batch=batch)
            adj_pool, _ = self.connect(edge_index=adj, so=so, edge_weight=edge_weight, batch=batch,
                                       batch_pooled=batch_pooled)
            if not self.sparse_output:
                return PoolingOutput(x=x_pool, edge_index=adj_pool, so=so)
            x_pool, ei, ew, batch_pooled = self._finalize_sparse_output(x_pool=x_pool, adj_pool=adj_pool, batch=batch,
                                                                        batch_pooled=batch_pooled, so=so)
            return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pooled, so=so)
        so = self.select(x=x, edge_index=adj, edge_weight=edge_weight, batch=batch, num_nodes=x.size(0))
        x_pool, batch_pooled = self.reduce(x=x, so=so, batch=batch, return_batched=not self.sparse_output)
        ei, ew = self.connect(edge_index=adj, so=so, edge_weight=edge_weight, batch=batch, batch_pooled=batch_pooled)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pooled, so=so)

    def extra_repr_args(self) -> dict:
        return {"batched": self.batched}


# =============================================================================== factory
# ("dmon", "kmis", "acc", "hosc", "bnpool", "jb" (JustBalancePooling), "edgepool" (EdgeContractionPooling), "lap" (LaPooling), "sag" (SAGPooling), "asap" (ASAPooling), "maxcut" (MaxCutPooling), "eigen" (EigenPooling), "nmf" (NMFPooling), "pan" (PANPooling) and "sep" (SEPPooling) are not in pooler_map yet: the alias set is pinned to the five poolers above)
pooler_classes = ["ASAPooling", "AsymCheegerCutPooling", "BNPool", "DMoNPooling", "DiffPool", "EdgeContractionPooling", "EigenPooling", "GraclusPooling", "HOSCPooling", "JustBalancePooling", "KMISPooling", "LaPooling", "MaxCutPooling", "MinCutPooling", "NDPPooling", "NMFPooling", "PANPooling", "SAGPooling", "SEPPooling", "TopkPooling"]

pooler_map = {
    "diff": DiffPool,
    "graclus": GraclusPooling,
    "mincut": MinCutPooling,
    "ndp": NDPPooling,
    "topk": TopkPooling,
}


def _missing_required(cls, given: dict) -> List[str]:
    out = []
    for name, p in inspect.signature(cls.__init__).parameters.items():
        if name == "self" or p.kind in (p.VAR_POSITIONAL, p.VAR_KEYWORD):
            continue
        if p.default is p.empty and name not in given:
            out.append(name)
    return out


def get_pooler(pooler_name: str, **kwargs):
    """Build a pooler from its alias (reference poolers/__init__.py:91-147): case-insensitive, a ``_u``
    suffix selects the unbatched mode, kwargs the constructor does not take are dropped silently, a
    missing required argument raises ``TypeError``."""
    alias = pooler_name.lower()
    if alias.endswith("_u") and alias[:-2] in pooler_map:
        alias = alias[:-2]
        kwargs.setdefault("batched", False)
    if alias not in pooler_map:
        raise ValueError(f"Unknown pooler_name='{pooler_name.lower()}'. "
                         f"Available poolers: {list(pooler_map.keys())}")
    cls = pooler_map[alias]
    sig = cls.get_signature()
    init_kwargs = kwargs if sig.has_kwargs else {k: v for k, v in kwargs.items() if k in sig.args}
    missing = _missing_required(cls, init_kwargs)
    if missing:
        raise TypeError(f"Missing required argument(s) for pooler '{alias}' ({cls.__name__}): "
                        f"{', '.join(missing)}")
    return cls(**init_kwargs)


__all__ = ["get_pooler", "pooler_map", "pooler_classes"] + pooler_classes + ["MaxCutSelect", "MaxCutScoreNet", "EigenPoolSelect",
                                                                          "EigenPoolReduce", "EigenPoolConnect",
                                                                          "EigenPoolLift", "NMFSelect", "SEPSelect"]
