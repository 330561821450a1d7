"""``AggrReduce``: pooled features from an aggregation operator (the interface of reference tgp/reduce/aggr_reduce.py)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _native as N
from ..select import SelectOutput
from ..utils.ops import batch_info, build_pooled_batch
from .aggr import _padded_ptr, is_aggregation, native_ops, native_readout, one_group_ptr
from .base_reduce import Reduce

_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _call_sorted(aggr, rows: Tensor, index: Tensor, groups: int) -> Tensor:
    """The composed route: the module sees its rows in ascending index order (a stable sort keeps the row order inside
    a group), as aggregations that need sorted input expect."""
    index, order = index.sort(stable=True)
    return aggr(rows.index_select(0, order), index=index, dim_size=groups, dim=0)


class AggrReduce(Reduce):
    r"""Reduce operator that wraps an aggregation module: a sparse :class:`~tgp.select.SelectOutput` aggregates
    ``x[node_index] * weight`` by ``cluster_index``; ``so=None`` is the graph-level readout over ``batch`` (or over the
    node dimension of a dense ``[B, N, F]``).  Dense assignments are refused, as in the reference.

    With :class:`~tgp.reduce.SumAggregation`, ``Mean``, ``Max``, ``Min`` or a ``MultiAggregation`` of them, float32 /
    half / bfloat16 device tensors are reduced by one pass of the segment readout kernel: no sort, no ``[nnz, F]``
    product, no ``x[mask]`` copy.  float64 tensors, an unsorted ``batch`` and any other aggregation module run the
    composed route (stable sort by index, then the module's own ``forward``).
    """

    def __init__(self, aggr):
        super().__init__()
        if not is_aggregation(aggr):
            raise TypeError(f"aggr must be a PyG Aggregation, got {type(aggr)}")
        self.aggr = aggr

    def _kernel_ops(self, x: Tensor):
        """The operations the readout kernel computes for this module and tensor; None: the composed route."""
        ops = native_ops(self.aggr)
        if ops is None:
            return None
        N.require_device(x)  # (the native aggregations have no CPU fallback)
        return ops if x.dtype in _KERNEL_DTYPES and x.size(-1) > 0 else None

    def forward(self, x: Tensor, so: Optional[SelectOutput] = None, *, batch: Optional[Tensor] = None,
                size: Optional[int] = None, **kwargs) -> Tuple[Tensor, Optional[Tensor]]:
        if so is None:
            return self._readout(x, batch, size)
        if not so.s.is_sparse:
            raise ValueError("AggrReduce supports only sparse SelectOutput assignments. "
                             "Dense assignments are not supported; use BaseReduce for dense/soft reductions.")
        batch = so.batch if batch is None else batch
        weight = so.weight
        ops = self._kernel_ops(x) if x.dim() == 2 and weight.dtype in _KERNEL_DTYPES else None
        if ops is not None:
            # a clustering's values are ones (known, not probed): the kernel then skips the weight load per row
            unit = bool(so.__dict__.get("_unit_values")) and not weight.requires_grad and weight.dtype == x.dtype
            x_pool = native_readout(x, ops, so.num_supernodes, so.assign_index().max_members, ("so", so),
                                    weight=None if unit else weight)
            return x_pool, self.reduce_batch(so, batch)
        x_pool = _call_sorted(self.aggr, x[so.node_index] * weight.view(-1, 1), so.cluster_index, so.num_supernodes)
        if batch is not None and not batch.is_cuda:  # (a user module on host tensors: reduce_batch is a kernel)
            batch_pool = torch.arange(so.num_supernodes, dtype=batch.dtype)
            batch_pool[so.cluster_index] = batch[so.node_index]
            return x_pool, batch_pool
        return x_pool, self.reduce_batch(so, batch)

    def _readout_dense(self, x: Tensor, mask: Optional[Tensor], ops) -> Tensor:
        """[B, N, F] (+ [B, N] mask, read by the kernel) -> [B, n_ops * F]."""
        B, Nn, F = x.shape
        m = None
        if mask is not None:
            m = (mask if mask.dtype == torch.bool else mask != 0).reshape(-1).contiguous().view(torch.uint8)
        return native_readout(x.reshape(B * Nn, F), ops, B, Nn, ("dense", Nn, m))

    def _readout(self, x: Tensor, batch: Optional[Tensor], size: Optional[int]) -> Tuple[Tensor, Optional[Tensor]]:
        """``so=None``: one output row per graph."""
        if x.dim() not in (2, 3):
            raise ValueError(f"Readout mode expects x to be 2D [N, F] or 3D [B, N, F], got ndim={x.dim()}.")
        if x.dim() == 3:
            B, Nn, F = x.shape
            groups = B if size is None else size
            ops = self._kernel_ops(x) if groups == B and B * Nn > 0 else None
            if ops is not None:
                x_pool = self._readout_dense(x, None, ops)
            else:
                x_pool = _call_sorted(self.aggr, x.reshape(B * Nn, F), build_pooled_batch(B, Nn, x.device), groups)
            return x_pool, torch.arange(groups, device=x.device)
        ops = self._kernel_ops(x)
        if batch is None:
            if ops is not None:
                return native_readout(x, ops, 1, x.size(0), ("ptr", one_group_ptr(x.size(0), x.device), None)), None
            return _call_sorted(self.aggr, x, x.new_zeros(x.size(0), dtype=torch.long), 1), None
        info = batch_info(batch) if ops is not None and batch.numel() > 0 and batch.is_cuda else None
        if size is not None:
            groups = size
        elif info is not None:
            groups = info.num_graphs
        else:  # a batch vector without nodes still stands for one graph (an all-false mask)
            groups = int(batch.max()) + 1 if batch.numel() > 0 else 1
        if info is not None and info.is_sorted and info.num_graphs <= groups:
            x_pool = native_readout(x, ops, groups, info.max_nodes, ("ptr", _padded_ptr(info, groups), N.i64c(batch)))
        else:
            x_pool = _call_sorted(self.aggr, x, batch, groups)
        return x_pool, torch.arange(groups, device=batch.device)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(aggr={self.aggr})"
