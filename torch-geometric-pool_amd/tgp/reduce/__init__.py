"""``reduce`` operators (reference tgp/reduce/): pooled features X' = S^T X (``BaseReduce``), aggregation-based
reduction and graph-level readout (``AggrReduce``, ``GlobalReduce``) and the aggregation operators they wrap.

Aggregator aliases of :func:`get_aggr`: ``sum``, ``mean``, ``max``, ``min`` and ``multi`` are built here on the
segment readout kernel; the reference's parametrised aliases resolve only when PyG is installed."""
from .aggr import (Aggregation, MaxAggregation, MeanAggregation, MinAggregation, MultiAggregation, SumAggregation)
from .aggr_reduce import AggrReduce
from .base_reduce import BaseReduce, Reduce, _DenseReduceFn, _SparseReduceFn  # noqa: F401
from .get_aggr import get_aggr, resolve_reduce_op
from .global_reduce import GlobalReduce

__all__ = ["Reduce", "BaseReduce", "AggrReduce", "GlobalReduce", "get_aggr", "resolve_reduce_op", "Aggregation",
           "SumAggregation", "MeanAggregation", "MaxAggregation", "MinAggregation", "MultiAggregation", "EigenPoolReduce"]


def __getattr__(name):
    # EigenPool's Reduce lives next to its pooler (tgp/poolers/eigenpool.py), which imports this package
    if name == "EigenPoolReduce":
        from ..poolers import eigenpool
        return eigenpool.EigenPoolReduce
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
