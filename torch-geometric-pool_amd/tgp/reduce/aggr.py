"""Aggregation operators with PyG's call form ``aggr(x, index=None, ptr=None, dim_size=None, dim=0)``.

``Sum`` / ``Mean`` / ``Max`` / ``Min`` / ``MultiAggregation`` have PyG's ``scatter`` semantics (an empty group gives 0,
the mean divides by ``max(count, 1)``) and run as ONE pass of the segment readout kernel (csrc/segment_aggr.hip) for
float32 / half / bfloat16 device tensors whose ``index`` is sorted; float64 and unsorted indices take the composed
``index_add_`` / ``scatter_reduce_`` form on the device.  Host tensors raise: there is no CPU fallback.  A user module
deriving from :class:`Aggregation` is called as written, wherever its tensors live.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from .. import _native as N
from .. import functions as Fn
from .. import kernels as K
from ..utils.ops import as_compute_dtype, batch_info

try:  # PyG is optional: when it is importable its plain aggregations are recognised by class and take the native route
    from torch_geometric.nn import aggr as _pyg_aggr
    if not isinstance(getattr(_pyg_aggr, "Aggregation", None), type):
        _pyg_aggr = None
except Exception:
    _pyg_aggr = None


class Aggregation(nn.Module):
    """Base class: ``forward(x, index, ptr, dim_size, dim)`` reduces ``x`` along ``dim`` into ``dim_size`` groups."""

    def forward(self, x: Tensor, index: Optional[Tensor] = None, ptr: Optional[Tensor] = None,
                dim_size: Optional[int] = None, dim: int = 0) -> Tensor:
        raise NotImplementedError

    def reset_parameters(self):
        pass

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}()"


def composed_aggregate(x: Tensor, index: Tensor, dim_size: int, op: str) -> Tensor:
    """PyG's ``scatter(x, index, 0, dim_size, op)`` from torch ops, in the dtype and on the device of ``x``: the same
    values.  The gradient of max / min departs from it in one case, on purpose: a group whose extreme is exactly 0 hands
    each tied row 1 / ties, as the kernel's backward does, where ``scatter_reduce`` started from zeros hands out
    1 / (ties + 1) ("Readout gradients at a zero extreme")."""
    out = x.new_zeros((dim_size,) + tuple(x.shape[1:]))
    if op in ("sum", "mean"):
        out.index_add_(0, index, x)
        if op == "mean":
            count = x.new_zeros(dim_size).index_add_(0, index, x.new_ones(index.numel())).clamp(min=1)
            out = out / count.view((-1,) + (1,) * (x.dim() - 1))
        return out
    # the extremes start from -inf / +inf: ATen's backward counts the initial value among the tied entries even with
    # include_self=False, so from zeros a group whose extreme is exactly 0 would hand its rows 1 / (ties + 1) of the
    # gradient, where the kernel's backward (and every other group) hands out 1 / ties
    shape = (-1,) + (1,) * (x.dim() - 1)
    idx = index.view(shape).expand_as(x)
    start = torch.full_like(out, float("-inf") if op == "max" else float("inf"))
    ext = start.scatter_reduce_(0, idx, x, reduce="amax" if op == "max" else "amin", include_self=False)
    some = torch.zeros(dim_size, dtype=torch.bool, device=x.device).index_fill_(0, index, True)
    return torch.where(some.view(shape), ext, out)


def _columns(out: Tensor, computed: Sequence[str], wanted: Sequence[str]) -> Tensor:
    """``out`` holds one column block per op of ``computed``; hand out the blocks of ``wanted``, in that order."""
    if list(computed) == list(wanted):
        return out
    F = out.size(-1) // len(computed)
    return torch.cat([out[..., computed.index(op) * F:(computed.index(op) + 1) * F] for op in wanted], dim=-1)


def native_readout(x: Tensor, ops: Sequence[str], num_groups: int, max_len: int, src, weight: Optional[Tensor] = None):
    """The kernel route: ``x`` [rows, F] on the device, fp32 arithmetic; the result has the dtype of ``x`` or, with
    assignment weights, the dtype the product ``x * weight`` promotes to."""
    computed = [op for op in K.SEGMENT_OPS if op in ops]
    w = None if weight is None else weight.float()
    out = Fn.segment_aggr(as_compute_dtype(x), K.segment_ops_mask(ops), num_groups, max_len, src, weight=w)
    out = _columns(out, computed, list(ops))
    want = x.dtype if weight is None else torch.promote_types(x.dtype, weight.dtype)
    return out if out.dtype == want else out.to(want)


_ONE_GROUP_PTR: dict = {}


def one_group_ptr(rows: int, device) -> Tensor:
    """``[0, rows]`` on the device: the offsets of a readout without a batch vector (the last few are kept)."""
    key = (int(rows), torch.device(device))
    hit = _ONE_GROUP_PTR.get(key)
    if hit is None:
        if len(_ONE_GROUP_PTR) >= 8:
            _ONE_GROUP_PTR.clear()
        hit = _ONE_GROUP_PTR[key] = torch.tensor([0, rows], dtype=torch.long, device=device)
    return hit


def aggregate(x: Tensor, ops: Sequence[str], index: Optional[Tensor] = None, ptr: Optional[Tensor] = None,
              dim_size: Optional[int] = None, dim: int = 0) -> Tensor:
    """What the five native classes compute; ``ops`` side by side on the last dimension."""
    N.require_device(x, index, ptr)
    if dim < 0:
        dim += x.dim()
    if not 0 <= dim < x.dim():
        raise ValueError(f"Encountered invalid dimension '{dim}' of source tensor with {x.dim()} dimensions")
    if ptr is not None and index is None:  # groups given by their offsets (PyG's segment form)
        ptr = ptr.to(torch.long)
        index = torch.repeat_interleave(torch.arange(ptr.numel() - 1, device=ptr.device), ptr[1:] - ptr[:-1])
        dim_size = ptr.numel() - 1 if dim_size is None else dim_size
    if index is None:  # every row in one group
        index = torch.zeros(x.size(dim), dtype=torch.long, device=x.device)
        dim_size = 1 if dim_size is None else dim_size
    if index.dim() != 1 or index.numel() != x.size(dim):
        raise ValueError("index must be one-dimensional with one entry per row of x along dim")
    if dim_size is None:
        dim_size = int(index.max()) + 1 if index.numel() > 0 else 0
    native = (x.dim() == 2 and dim == 0 and x.dtype in (torch.float32, torch.float16, torch.bfloat16)
              and x.size(1) > 0)
    if native and index.numel() > 0:
        info = batch_info(index)
        native = info.is_sorted and info.num_graphs <= dim_size
    if native:
        if index.numel() == 0:
            seg, longest = torch.zeros(dim_size + 1, dtype=torch.long, device=x.device), 0
        else:
            seg, longest = _padded_ptr(info, dim_size), info.max_nodes
        return native_readout(x, ops, dim_size, longest, ("ptr", seg, N.i64c(index)))
    xt = x.movedim(dim, 0)
    return torch.cat([composed_aggregate(xt, index, dim_size, op).movedim(0, dim) for op in ops], dim=-1)


def _padded_ptr(info, dim_size: int) -> Tensor:
    """The offsets of a sorted batch vector, with the groups beyond its last id (``size``) empty at the end."""
    extra = dim_size - info.num_graphs
    return info.ptr if extra == 0 else torch.cat([info.ptr, info.ptr[-1:].expand(extra)])


class _NativeAggregation(Aggregation):
    op: str = ""

    def forward(self, x: Tensor, index: Optional[Tensor] = None, ptr: Optional[Tensor] = None,
                dim_size: Optional[int] = None, dim: int = 0) -> Tensor:
        return aggregate(x, (self.op,), index, ptr, dim_size, dim)


class SumAggregation(_NativeAggregation):
    op = "sum"


class MeanAggregation(_NativeAggregation):
    op = "mean"


class MaxAggregation(_NativeAggregation):
    op = "max"


class MinAggregation(_NativeAggregation):
    op = "min"


class MultiAggregation(Aggregation):
    """Several aggregations side by side on the last dimension (``mode="cat"``).  Members are aliases of
    :func:`tgp.reduce.get_aggr` or instances; when all of them are sum / mean / max / min they cost one pass over ``x``."""

    def __init__(self, aggrs, aggrs_kwargs: Optional[List[dict]] = None, mode: Optional[str] = "cat",
                 mode_kwargs: Optional[dict] = None):
        super().__init__()
        if not isinstance(aggrs, (list, tuple)):
            raise ValueError(f"'aggrs' of '{self.__class__.__name__}' should be a list or tuple (got '{type(aggrs)}').")
        if len(aggrs) == 0:
            raise ValueError(f"'aggrs' of '{self.__class__.__name__}' should not be empty.")
        if mode != "cat":
            raise NotImplementedError(f"MultiAggregation: only mode='cat' is built here (got mode={mode!r})")
        if aggrs_kwargs is None:
            aggrs_kwargs = [{}] * len(aggrs)
        elif len(aggrs) != len(aggrs_kwargs):
            raise ValueError(f"'aggrs_kwargs' with invalid length passed to '{self.__class__.__name__}' (got "
                             f"'{len(aggrs_kwargs)}', expected '{len(aggrs)}').")
        from .get_aggr import get_aggr
        self.aggrs = nn.ModuleList([get_aggr(a, **kw) if isinstance(a, str) else a for a, kw in zip(aggrs, aggrs_kwargs)])
        self.mode = mode

    def reset_parameters(self):
        for aggr in self.aggrs:
            if hasattr(aggr, "reset_parameters"):
                aggr.reset_parameters()

    def forward(self, x: Tensor, index: Optional[Tensor] = None, ptr: Optional[Tensor] = None,
                dim_size: Optional[int] = None, dim: int = 0) -> Tensor:
        ops = native_ops(self)
        if ops is not None:
            return aggregate(x, ops, index, ptr, dim_size, dim)
        return torch.cat([aggr(x, index=index, ptr=ptr, dim_size=dim_size, dim=dim) for aggr in self.aggrs], dim=-1)

    def __repr__(self) -> str:
        aggrs = ",\n".join(f"  {aggr}" for aggr in self.aggrs) + ",\n"
        return f"{self.__class__.__name__}([\n{aggrs}], mode={self.mode})"


_NATIVE_CLASS_NAMES = {"SumAggregation": "sum", "MeanAggregation": "mean", "MaxAggregation": "max",
                       "MinAggregation": "min"}


def native_ops(aggr) -> Optional[Tuple[str, ...]]:
    """The operations of an aggregation the readout kernel computes itself, in output order; None for any other."""
    if isinstance(aggr, _NativeAggregation):
        return (aggr.op,)
    if isinstance(aggr, MultiAggregation):
        members = [native_ops(a) for a in aggr.aggrs]
        return None if any(m is None for m in members) else tuple(op for m in members for op in m)
    if _pyg_aggr is not None:
        for name, op in _NATIVE_CLASS_NAMES.items():
            if type(aggr) is getattr(_pyg_aggr, name, None):
                return (op,)
        if type(aggr) is getattr(_pyg_aggr, "MultiAggregation", None) and getattr(aggr, "mode", None) == "cat":
            members = [native_ops(a) for a in aggr.aggrs]
            return None if any(m is None for m in members) else tuple(op for m in members for op in m)
    return None


def is_aggregation(obj) -> bool:
    """An instance of :class:`Aggregation`, or of PyG's base class when PyG is importable."""
    return isinstance(obj, Aggregation) or (_pyg_aggr is not None and isinstance(obj, _pyg_aggr.Aggregation))
