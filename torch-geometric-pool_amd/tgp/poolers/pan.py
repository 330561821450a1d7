"""PAN pooling (Ma et al., NeurIPS 2020; reference poolers/pan.py): top-k pooling over the score

    score = beta[0] * (x . p) + beta[1] * colsum(M)

with ``M`` the maximal-entropy-transition matrix a :class:`tgp.nn.PANConv` returned.  Select is ``TopkSelect`` (without
a projection of its own), Reduce ``BaseReduce``, Connect ``SparseConnect`` on ``M`` itself, Lift ``BaseLift``.

Routes.  Device float32 inputs in ratio mode with a tanh or linear activation take ``tgp_pan_score_f32``:
one launch over the by-column group index of ``M``, the activation fused, the result handed straight to the device
selection.  ``min_score``, other activations and other dtypes compose the same score from torch operators on the device.
An ``M`` that came from ``PANConv`` brings its record along (CSR offsets, the group index once built): nothing the
convolution already knew is built again.  Host tensors are refused: there is no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional, Union

import torch
from torch import Tensor
from torch.nn import Parameter

from .. import _native as N
from .. import functions as Fn
from .. import kernels as K
from ..connect import SparseConnect
from ..imports import is_sparsetensor
from ..lift import BaseLift
from ..reduce import BaseReduce
from ..select import SelectOutput, TopkSelect
from ..src import PoolingOutput, SRCPooling


class PANPooling(SRCPooling):
    r"""The path integral based pooling operator from `"Path Integral Based Convolution and Pooling for Graph Neural
    Networks" <https://arxiv.org/abs/2006.16811>`_ (reference poolers/pan.py:18-211): the same constructor arguments and
    defaults, ``p`` filled with 1 and ``beta`` with 0.5.

    ``adj`` is the MET matrix from :class:`tgp.nn.PANConv`: a torch sparse COO or CSR tensor ``[N, N]``, or a
    ``torch_sparse.SparseTensor`` when that package is installed.  The reference asserts ``HAS_TORCH_SPARSE``; this
    build has no such dependency and does not.  The output carries ``edge_index = adj_pool`` in the format ``adj`` came
    in and ``edge_weight = None``, as the reference's does.

    The ``"pan"`` alias of ``get_pooler`` is not registered (the alias set is pinned to the five hot-path poolers)."""

    def __init__(self, in_channels: int, ratio: float = 0.5, min_score: Optional[float] = None, multiplier: float = 1.0,
                 nonlinearity: Union[str, Callable] = "tanh", lift: str = "precomputed", s_inv_op: str = "transpose",
                 connect_red_op: str = "sum", lift_red_op: str = "sum", remove_self_loops: bool = False,
                 degree_norm: bool = False, edge_weight_norm: bool = False):
        super().__init__(
            selector=TopkSelect(ratio=ratio, min_score=min_score, act=nonlinearity, s_inv_op=s_inv_op),
            reducer=BaseReduce(),
            lifter=BaseLift(matrix_op=lift, reduce_op=lift_red_op),
            connector=SparseConnect(remove_self_loops=remove_self_loops, reduce_op=connect_red_op,
                                    degree_norm=degree_norm, edge_weight_norm=edge_weight_norm))
        self.in_channels = in_channels
        self.ratio = ratio
        self.min_score = min_score
        self.multiplier = multiplier
        self.p = Parameter(torch.empty(in_channels))
        self.beta = Parameter(torch.empty(2))
        self.reset_own_parameters()

    def reset_own_parameters(self):
        r"""Resets :math:`p` and :math:`\beta`."""
        self.p.data.fill_(1)
        self.beta.data.fill_(0.5)

    def reset_parameters(self):
        self.reset_own_parameters()
        super().reset_parameters()

    @staticmethod
    def _met_of(adj, n: int):
        """(the MET record of ``adj``, ``adj`` as a coalesced torch COO tensor)."""
        if is_sparsetensor(adj):  # pragma: no cover  (torch_sparse is not a dependency of this build)
            row, col, value = adj.coo()
            assert value is not None
            adj = torch.sparse_coo_tensor(torch.stack([row, col]), value, (n, n), is_coalesced=True)
        if not isinstance(adj, Tensor) or adj.layout == torch.strided:
            raise ValueError("PANPooling: adj must be the MET matrix of PANConv as a torch sparse COO / CSR tensor (or a "
                             f"torch_sparse.SparseTensor), got {type(adj).__name__}")
        met = K.pan_record(adj)
        if met is not None:
            return met, adj
        coo = adj if adj.layout == torch.sparse_coo else adj.to_sparse_coo()
        coo = coo if coo.is_coalesced() else coo.coalesce()
        index, values = coo.indices(), coo.values()
        row_ptr = K.csr_offsets(index, n) if index.is_cuda and values.dtype == torch.float32 else None
        met = K.PanMet(index, values, row_ptr, n)
        if row_ptr is not None:
            K.pan_remember(adj, met)
        return met, coo

    def _score_and_select(self, x: Tensor, met, batch: Optional[Tensor]) -> SelectOutput:
        sel = self.selector
        if (type(sel) is TopkSelect and sel.min_score is None and sel.ratio is not None and sel._fused_act is not None
                and self._so_cached is None and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.size(0) > 0
                and met.values.dtype == torch.float32 and self.p.dtype == torch.float32):
            # ratio mode, tanh or linear: the activation rides in the score kernel and the score goes straight to the
            # device selection (under autograd the scorer is one graph node; so.weight reaches it through take_unique)
            score = Fn.pan_score(x, self.p, self.beta, met, sel._fused_act == "tanh")
            return sel._native_select(score, batch, x.size(0))
        score1 = (x * self.p).sum(dim=-1)
        score2 = torch.zeros(x.size(0), dtype=met.values.dtype, device=x.device).index_add(0, met.index[1], met.values)
        return self.select(x=(self.beta[0] * score1 + self.beta[1] * score2).view(-1, 1), batch=batch)

    def forward(self, x: Tensor, adj=None, so: Optional[SelectOutput] = None, batch: Optional[Tensor] = None,
                lifting: bool = False, **kwargs):
        if lifting:
            return self.lift(x_pool=x, so=so)
        met, coo = self._met_of(adj, x.size(0))
        N.require_device(x, met.values, batch)
        so = self._score_and_select(x, met, batch)
        x_pool, batch_pooled = self.reduce(x=x, so=so, batch=batch)
        if self.multiplier != 1:
            x_pool = self.multiplier * x_pool
        adj_pool, _ = self.connect(edge_index=coo, so=so, batch_pooled=batch_pooled)
        if is_sparsetensor(adj):  # pragma: no cover
            from ..utils.ops import connectivity_to_sparsetensor
            adj_pool = connectivity_to_sparsetensor(adj_pool, None, so.num_supernodes)
        elif adj.layout == torch.sparse_csr:
            adj_pool = adj_pool.to_sparse_csr()
        return PoolingOutput(x=x_pool, edge_index=adj_pool, edge_weight=None, batch=batch_pooled, so=so)

    def extra_repr_args(self) -> dict:
        return {"multiplier": self.multiplier}
