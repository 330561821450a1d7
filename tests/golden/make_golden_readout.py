#!/usr/bin/env python3
"""Generate the golden vectors of the aggregation readout (``tests/golden/golden_readout_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_sag.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs ``AggrReduce``,
``GlobalReduce`` and ``get_aggr`` on small seeded inputs.  The stand-in sets ``torch_geometric.nn.aggr.Aggregation`` to
``None``, so the five aggregation classes the reference resolves (``Sum`` / ``Mean`` / ``Max`` / ``Min`` /
``MultiAggregation``) are defined HERE over the stand-in's ``scatter``, the way PyG's ``Aggregation.reduce`` calls it,
and installed into the stand-in's module before the reference is imported.  ``pyg_shim.py`` itself is not touched.

The limit README.md states for every "bit-exact" claim applies here too: the reference's own code produced these
vectors, but the PyG leaves underneath it (``scatter`` and the aggregation classes) are restated from their published
behaviour, and a shared misreading of a leaf would pass both sides.

Every case stores the float32 run, a float64 run, and the float64 gradients of ``sum(out ** 2)`` with respect to ``x``
(and to the assignment weights).  The gradient run hands the reference's ``AggrReduce`` an object with the fields of a
``SelectOutput`` it reads, so that the weights are a leaf tensor.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_readout.py
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import torch  # noqa: E402

import pyg_shim  # noqa: E402

pyg_shim.install()


class Aggregation(torch.nn.Module):
    """PyG's base class, as far as the reference uses it: ``reduce`` is ``scatter`` along ``dim``."""

    def reset_parameters(self):
        pass

    def reduce(self, x, index, dim_size, dim, reduce):
        return pyg_shim.scatter(x, index, dim, dim_size, reduce)

    def __repr__(self):
        return f"{self.__class__.__name__}()"


def _plain(name):
    def forward(self, x, index=None, ptr=None, dim_size=None, dim=-2):
        return self.reduce(x, index, dim_size, dim, name)
    return forward


SumAggregation = type("SumAggregation", (Aggregation,), {"forward": _plain("sum")})
MeanAggregation = type("MeanAggregation", (Aggregation,), {"forward": _plain("mean")})
MaxAggregation = type("MaxAggregation", (Aggregation,), {"forward": _plain("max")})
MinAggregation = type("MinAggregation", (Aggregation,), {"forward": _plain("min")})
_BY_NAME = {"sum": SumAggregation, "mean": MeanAggregation, "max": MaxAggregation, "min": MinAggregation}


class MultiAggregation(Aggregation):
    def __init__(self, aggrs, mode="cat"):
        super().__init__()
        assert mode == "cat"
        self.aggrs = torch.nn.ModuleList([_BY_NAME[a]() if isinstance(a, str) else a for a in aggrs])

    def forward(self, x, index=None, ptr=None, dim_size=None, dim=-2):
        return torch.cat([a(x, index=index, ptr=ptr, dim_size=dim_size, dim=dim) for a in self.aggrs], dim=-1)


_aggr = sys.modules["torch_geometric.nn.aggr"]
sys.modules["torch_geometric.nn"].aggr = _aggr  # (`from torch_geometric.nn import aggr` reads the attribute)
for _cls in (Aggregation, SumAggregation, MeanAggregation, MaxAggregation, MinAggregation, MultiAggregation):
    setattr(_aggr, _cls.__name__, _cls)

import make_golden as G  # noqa: E402  (imports the reference over the stand-in)
from tgp.reduce import AggrReduce, GlobalReduce, get_aggr  # noqa: E402
from tgp.select import SelectOutput  # noqa: E402

OPS = {"sum": {}, "mean": {}, "max": {}, "min": {}, "multi": {"aggrs": ["sum", "mean", "max"]}}
CASES = {}


def batch_of(sizes):
    return torch.cat([torch.full((n,), g, dtype=torch.long) for g, n in enumerate(sizes)])


def inputs_batch(gen):
    sizes = torch.randint(8, 25, (4,), generator=gen).tolist()
    return dict(x=torch.randn(sum(sizes), 5, generator=gen), batch=batch_of(sizes))


def inputs_batch_size(gen):
    d = inputs_batch(gen)
    d["size"] = 6  # two trailing graphs without nodes
    return d


def inputs_no_batch(gen):
    return dict(x=torch.randn(12, 5, generator=gen))


def inputs_dense(gen):
    return dict(x=torch.randn(3, 7, 4, generator=gen))


def inputs_dense_masked(gen):
    mask = torch.rand(3, 7, generator=gen) < 0.6
    mask[1] = False  # a graph without nodes
    mask[0, 0], mask[0, 3], mask[2, 6] = True, False, True
    return dict(x=torch.randn(3, 7, 4, generator=gen), mask=mask)


def inputs_so_topk(gen):
    """One member per supernode, with weights (TopK-shaped); node_index ascending as a selector leaves it."""
    nodes = torch.randperm(20, generator=gen)[:8].sort().values
    return dict(x=torch.randn(20, 5, generator=gen), node_index=nodes, cluster_index=torch.randperm(8, generator=gen),
                weight=torch.rand(8, generator=gen) + 0.1, num_nodes=20, num_supernodes=8, batch=None)


def inputs_so_pairs(gen):
    """Unit pairs in no order (Graclus-shaped), two graphs."""
    cluster = torch.cat([torch.arange(4).repeat(2)[torch.randperm(8, generator=gen)][:7],
                         4 + torch.arange(3).repeat(2)[torch.randperm(6, generator=gen)]])
    return dict(x=torch.randn(13, 5, generator=gen), node_index=torch.arange(13), cluster_index=cluster, weight=None,
                num_nodes=13, num_supernodes=7, batch=batch_of([7, 6]))


def inputs_so_empty(gen):
    """Supernodes 2 and 4 have no member; the others two to four, weighted."""
    cluster = torch.tensor([0, 1, 3, 5])[torch.randint(0, 4, (10,), generator=gen)]
    return dict(x=torch.randn(10, 5, generator=gen), node_index=torch.arange(10), cluster_index=cluster,
                weight=torch.rand(10, generator=gen) + 0.1, num_nodes=10, num_supernodes=6, batch=None)


def select_output(i, dtype):
    w = None if i["weight"] is None else i["weight"].to(dtype)
    return SelectOutput(node_index=i["node_index"], cluster_index=i["cluster_index"], weight=w,
                        num_nodes=i["num_nodes"], num_supernodes=i["num_supernodes"])


def run(kind, op, i, dtype, grad=False):
    """(pooled x, pooled batch or None, gradients or None) of one reference call."""
    x = i["x"].to(dtype)
    if grad:
        x = x.clone().requires_grad_(True)
    leaves = [x]
    if kind == "global":
        out = GlobalReduce(op, **OPS[op])(x, batch=i.get("batch"), size=i.get("size"), mask=i.get("mask"))
        batch_pool = None
    else:
        reducer = AggrReduce(get_aggr(op, **OPS[op]))
        if "node_index" in i:
            so = select_output(i, dtype)
            if grad and i["weight"] is not None:  # the same fields, with the weights as a leaf
                w = so.weight.detach().clone().requires_grad_(True)
                leaves.append(w)
                so = types.SimpleNamespace(s=so.s, node_index=so.node_index, cluster_index=so.cluster_index, weight=w,
                                           num_supernodes=so.num_supernodes, batch=None)
            out, batch_pool = reducer(x, so, batch=i["batch"])
        else:
            out, batch_pool = reducer(x, batch=i.get("batch"), size=i.get("size"))
    grads = torch.autograd.grad((out ** 2).sum(), leaves) if grad else None
    return out, batch_pool, grads


def add_cases(name, kind, make_inputs, seed):
    for op in OPS:
        i = make_inputs(torch.Generator().manual_seed(seed))
        with torch.no_grad():
            out, batch_pool, _ = run(kind, op, i, torch.float32)
        out64, _, grads = run(kind, op, i, torch.float64, grad=True)
        f64 = {"x": G.t(out64), "grads": {"x": G.t(grads[0])}}
        if len(grads) > 1:
            f64["grads"]["weight"] = G.t(grads[1])
        CASES[f"{name}_{op}"] = {"kind": kind, "op": op, "op_kwargs": OPS[op], "seed": seed,
                                 "inputs": {k: G.t(v) for k, v in i.items()},
                                 "expected": {"x": G.t(out), "batch": G.t(batch_pool)}, "f64": f64}
    print(f"{name}: x {tuple(i['x'].shape)} -> {tuple(out.shape)}")


def main():
    add_cases("global_batch", "global", inputs_batch, 100)
    add_cases("aggr_batch_size", "aggr", inputs_batch_size, 110)
    add_cases("global_no_batch", "global", inputs_no_batch, 120)
    add_cases("aggr_no_batch", "aggr", inputs_no_batch, 125)
    add_cases("global_dense", "global", inputs_dense, 130)
    add_cases("aggr_dense", "aggr", inputs_dense, 135)
    add_cases("global_dense_masked", "global", inputs_dense_masked, 140)
    add_cases("aggr_so_topk", "aggr", inputs_so_topk, 150)
    add_cases("aggr_so_pairs", "aggr", inputs_so_pairs, 160)
    add_cases("aggr_so_empty", "aggr", inputs_so_empty, 170)
    out = os.path.join(HERE, "golden_readout_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
