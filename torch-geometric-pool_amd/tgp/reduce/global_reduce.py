"""``GlobalReduce``: graph-level readout as a module (the interface of reference tgp/reduce/global_reduce.py)."""
from __future__ import annotations

from typing import Optional, Union

from torch import Tensor

from ..utils.ops import apply_dense_node_mask
from .aggr_reduce import AggrReduce
from .get_aggr import resolve_reduce_op


class GlobalReduce(AggrReduce):
    r"""One vector per graph from ``[N, F]`` features with an optional ``batch`` vector, or from dense ``[B, N, F]``
    features with an optional boolean ``mask`` of shape ``[B, N]``.

    Args:
        reduce_op: a string alias of :func:`~tgp.reduce.get_aggr` (``"sum"``, ``"mean"``, ``"max"``, ``"min"``,
            ``"multi"``) or an Aggregation instance.
        **aggr_kwargs: passed to :func:`~tgp.reduce.get_aggr` when ``reduce_op`` is a string.
    """

    def __init__(self, reduce_op: Union[str, object] = "sum", **aggr_kwargs):
        super().__init__(resolve_reduce_op(reduce_op, **aggr_kwargs))

    def forward(self, x: Tensor, batch: Optional[Tensor] = None, size: Optional[int] = None,
                mask: Optional[Tensor] = None) -> Tensor:
        if x.dim() == 3:  # dense: `batch` and `size` are not read, the graphs are the rows of the first dimension
            if mask is None:
                return self._readout(x, None, x.size(0))[0]
            if tuple(mask.shape) != tuple(x.shape[:2]):
                raise ValueError("mask must have shape [B, N] matching x.shape[:2] for dense readout.")
            ops = self._kernel_ops(x) if x.size(0) * x.size(1) > 0 else None
            if ops is not None:  # the kernel reads the mask: no x[mask] copy
                return self._readout_dense(x, mask, ops)
            rows, row_batch = apply_dense_node_mask(x, mask)
            return self._readout(rows, row_batch, mask.size(0))[0]
        if x.dim() != 2:
            raise ValueError(f"readout expects x to be 2D [N, F] or 3D [B, N, F], got ndim={x.dim()}")
        if mask is not None:
            raise ValueError("mask is only supported for dense x with shape [B, N, F].")
        if size is not None and batch is None:
            raise ValueError("size is only supported for sparse readout when batch is provided.")
        return self._readout(x, batch, size)[0]
