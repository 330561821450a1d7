"""Resolve aggregation operators by alias (the interface of reference tgp/reduce/get_aggr.py).

``sum``, ``mean``, ``max``, ``min`` and ``multi`` resolve to the classes of :mod:`tgp.reduce.aggr`, which run on the
segment readout kernel.  The reference's other aliases name parametrised or learned PyG aggregators: they resolve to
PyG's class when ``torch_geometric`` is importable and raise ``NotImplementedError`` otherwise.
"""
from __future__ import annotations

import inspect
from typing import Any, Union

from . import aggr as _native_module
from .aggr import _pyg_aggr, is_aggregation

_NATIVE_CLASSES = {"sum": "SumAggregation", "mean": "MeanAggregation", "max": "MaxAggregation",
                   "min": "MinAggregation", "multi": "MultiAggregation"}
# the aliases only PyG can serve: "<alias>" names "<Alias>Aggregation" unless listed with another class name
_PYG_ONLY = ("mul var std softmax power_mean median quantile lstm gru degree_scaler sort attentional equilibrium mlp "
             "deep_sets set_transformer lcm variance_preserving patch_transformer set2set graph_multiset_transformer").split()
_PYG_OTHER_NAMES = {"set2set": "Set2Set", "graph_multiset_transformer": "GraphMultisetTransformer", "lstm":
                    "LSTMAggregation", "gru": "GRUAggregation", "mlp": "MLPAggregation", "lcm": "LCMAggregation"}


def _camel(alias: str) -> str:
    return "".join(part.capitalize() for part in alias.split("_")) + "Aggregation"


_AGGR_ALIASES = dict(_NATIVE_CLASSES)
_AGGR_ALIASES.update({a: _PYG_OTHER_NAMES.get(a, _camel(a)) for a in _PYG_ONLY})


def is_pyg_aggregation(obj: Any) -> bool:
    """:obj:`True` for an instance of :class:`tgp.reduce.Aggregation` or, with PyG importable, of PyG's base class."""
    return is_aggregation(obj)


def resolve_reduce_op(reduce_op: Union[str, Any], **kwargs: Any) -> Any:
    """A string alias goes through :func:`get_aggr`; an Aggregation instance is returned as it is."""
    if isinstance(reduce_op, str):
        return get_aggr(reduce_op, **kwargs)
    if not is_aggregation(reduce_op):
        raise TypeError(f"reduce_op must be a string alias or a PyG Aggregation instance, got {type(reduce_op)}")
    return reduce_op


def _accepted(cls, kwargs: dict) -> dict:
    """The keyword arguments the class's constructor names (all of them when its signature cannot be read)."""
    try:
        names = set(inspect.signature(cls.__init__).parameters) - {"self"}
    except (TypeError, ValueError):
        return dict(kwargs)
    return {k: v for k, v in kwargs.items() if k in names}


def get_aggr(alias: str, **kwargs: Any) -> Any:
    """Aggregation instance by alias.  Case-insensitive, dashes count as underscores; keyword arguments the class's
    ``__init__`` does not take are dropped, as in the reference."""
    key = alias.strip().lower().replace("-", "_")
    class_name = _AGGR_ALIASES.get(key)
    if class_name is None:
        raise ValueError(f"Unknown aggregator alias: {alias!r}. Known aliases: {sorted(_AGGR_ALIASES.keys())}")
    if key in _NATIVE_CLASSES:
        return getattr(_native_module, class_name)(**_accepted(getattr(_native_module, class_name), kwargs))
    if _pyg_aggr is None:
        raise NotImplementedError(
            f"Aggregator alias {key!r} ({class_name}) is a parametrised PyG aggregator that this build does not "
            f"restate; it resolves to PyG's class when torch_geometric is installed. Native aliases: "
            f"{sorted(_NATIVE_CLASSES)}")
    cls = getattr(_pyg_aggr, class_name, None)
    if cls is None:
        raise ValueError(f"Aggregator {class_name!r} not found in torch_geometric.nn.aggr. "
                         "Your PyG version may not include it.")
    if key in ("lstm", "gru") and "in_channels" in kwargs:  # PyG's recurrent aggregators want both channel counts
        kwargs.setdefault("out_channels", kwargs["in_channels"])
    return cls(**_accepted(cls, kwargs))
