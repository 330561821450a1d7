#!/usr/bin/env python3
"""Generate the golden vectors of k-MIS pooling (``tests/golden/golden_kmis_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_dmon.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs ``KMISPooling`` on
small seeded inputs.  The reference's ``kmis_select`` needs four leaves the stand-in does not have (torch_scatter's
``scatter_min`` / ``scatter_max`` / ``scatter_add`` with ``out=``, PyG's ``Linear``); they are supplied here, written
from the packages' published behaviour, by assigning into the imported reference module.

The reference's tie order is not a contract (its ``argsort`` is stable only up to 16 elements on the host), so a case is
kept only if
  (a) the reference's own ``argsort`` of its updated score equals the stable one (asserted),
and, for the linear scorer,
  (b) adjacent sorted updated scores differ by at least 1e-5 relative (the project's fp32 tolerance: rounding on another
      device cannot reorder such a case), and
  (c) the order computed in float64 is the same.
Seeds are walked until a case passes (b) and (c); the seed is stored.  Every case also stores a float64 run: scores,
pooled x and the gradients of ``sum(x_pool ** 2)`` with respect to ``x`` and the scorer's parameters.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kmis.py
"""
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as G  # noqa: E402  (installs the PyG stand-in and imports the reference)
import tgp.select.kmis_select as RK  # noqa: E402
from make_golden_dmon import directed_graphs  # noqa: E402


# ---- the leaves the stand-in lacks (torch_scatter 2.1.2 `out=` forms, torch_geometric.nn.dense.Linear) -------------
def _scatter_add(src, index, dim=-1, out=None, dim_size=None):
    if out is None:
        size = dim_size if dim_size is not None else (int(index.max()) + 1 if index.numel() else 0)
        out = src.new_zeros(size)
    return out.scatter_add_(0, index, src)


def _scatter_minmax(reduce):
    def fn(src, index, dim=-1, out=None, dim_size=None):
        if out is None:
            size = dim_size if dim_size is not None else (int(index.max()) + 1 if index.numel() else 0)
            out = src.new_zeros(size).scatter_reduce_(0, index, src, reduce=reduce, include_self=False)
        else:
            out.scatter_reduce_(0, index, src, reduce=reduce, include_self=True)
        return out, torch.full_like(index, -1)  # (the argument positions: nobody here reads them)
    return fn


class _Linear(torch.nn.Module):
    def __init__(self, in_channels, out_channels, bias=True, weight_initializer=None, bias_initializer=None):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = torch.nn.Parameter(torch.empty(out_channels, in_channels))
        self.bias = torch.nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.in_channels)
        torch.nn.init.uniform_(self.weight, -bound, bound)
        if self.bias is not None:
            torch.nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        return torch.nn.functional.linear(x, self.weight, self.bias)


RK.scatter_add = _scatter_add
RK.scatter_min = _scatter_minmax("amin")
RK.scatter_max = _scatter_minmax("amax")
RK.Linear = _Linear
RK.HAS_TORCH_SCATTER = True

from tgp.poolers.kmis import KMISPooling  # noqa: E402

CASES = {}


def updated_of(pooler, x, ei, ew, n):
    sel = pooler.selector
    score = sel._scorer(ei, ew, x, num_nodes=n)
    return sel._apply_heuristic(score, ei).reshape(-1)


def order_ok(pooler, inputs, linear):
    """(b), (c): False sends the caller to the next seed; (a) is asserted on what is kept."""
    import copy
    x, ei, ew = inputs["x"], inputs["edge_index"], inputs["edge_weight"]
    n = x.size(0)
    with torch.no_grad():
        upd = updated_of(pooler, x, ei, ew, n)
        as_float = upd if upd.is_floating_point() else upd.double()
        stable = torch.argsort(as_float, dim=0, descending=True, stable=True)
        if linear:
            s = upd[stable]
            gap = (s[:-1] - s[1:]) / s[:-1].abs().clamp_min(1e-30)
            if gap.numel() and float(gap.min()) < 1e-5:
                return False
            p64 = copy.deepcopy(pooler).double()
            upd64 = updated_of(p64, x.double(), ei, None if ew is None else ew.double(), n)
            if not torch.equal(torch.argsort(upd64, dim=0, descending=True, stable=True), stable):
                return False
        ref_perm = torch.argsort(upd, 0, descending=True)  # exactly the reference's call
        assert torch.equal(ref_perm, stable), "the reference's own order is not the stable one: not a usable case"
    return True


def f64_run(cfg, params, inputs):
    pooler = KMISPooling(**cfg).double().eval()
    pooler.load_state_dict({k: v.double() for k, v in params.items()})
    x = inputs["x"].double().clone().requires_grad_(True)
    ew = inputs["edge_weight"]
    out = pooler(x=x, adj=inputs["edge_index"], edge_weight=None if ew is None else ew.double(), batch=inputs["batch"])
    names = [n for n, _ in pooler.named_parameters()]
    leaves = [x] + [p for _, p in pooler.named_parameters()]
    g = torch.autograd.grad((out.x ** 2).sum(), leaves, allow_unused=True)
    return {"score": G.t(out.so.weight), "x": G.t(out.x),
            "grads": {"x": G.t(g[0] if g[0] is not None else torch.zeros_like(x)),
                      "params": {n: G.t(gi if gi is not None else torch.zeros_like(p))
                                 for n, gi, p in zip(names, g[1:], leaves[1:])}}}


def add_case(name, cfg, make_inputs, first_seed):
    linear = cfg.get("scorer", "linear") == "linear"
    for seed in range(first_seed, first_seed + 200):
        inputs = make_inputs(seed)
        torch.manual_seed(seed)
        pooler = KMISPooling(**cfg).eval()
        if order_ok(pooler, inputs, linear):
            break
    else:
        raise RuntimeError(f"{name}: no seed gave a tie-free, well-separated order")
    with torch.no_grad():
        out = pooler(x=inputs["x"], adj=inputs["edge_index"], edge_weight=inputs["edge_weight"], batch=inputs["batch"])
    params = G.params_of(pooler)
    exp = G.pool_dict(out)
    exp["so"]["mis"] = G.t(out.so.mis)
    del exp["so"]["node_index"]  # (0..N-1: the consumer rebuilds it)
    assert name not in CASES, name
    CASES[name] = {"kind": "pool", "seed": seed, "inputs": {k: G.t(v) for k, v in inputs.items()}, "params": params,
                   "cfg": cfg, "expected": exp, "f64": f64_run(cfg, params, inputs)}
    print(f"{name}: seed {seed}, N={inputs['x'].size(0)}, K={out.so.num_supernodes}")


def undirected_batch(seed, feat=4, p=0.08, four=False):
    gen = torch.Generator().manual_seed(seed)
    nb = int(torch.randint(4, 7, (1,), generator=gen))
    nb = 4 if four else nb
    sizes = torch.randint(5, 41, (nb,), generator=gen).tolist()
    x, ei, ew, batch = G.batched_graphs(sizes, p, gen, feat, True)
    return dict(x=x, edge_index=ei, edge_weight=ew, batch=batch)


def denser_batch(seed):
    """"w-greedy" ties every node without an incoming edge at exactly 1: graphs dense enough to have few of them."""
    return undirected_batch(seed, p=0.2, four=True)


def four_graphs(seed):
    return undirected_batch(seed, four=True)


def directed_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(5, 31, (4,), generator=gen).tolist()
    x, ei, ew, batch = directed_graphs(sizes, 0.12, gen, 4)
    return dict(x=x, edge_index=ei, edge_weight=ew, batch=batch)


def edgeless_batch(seed):
    d = four_graphs(seed)
    ei, ew, batch = d["edge_index"], d["edge_weight"], d["batch"]
    keep = (batch[ei[0]] != 1) & (ei[0] % 7 != 3) & (ei[1] % 7 != 3)  # graph 1 loses its edges, every 7th node its own
    d["edge_index"], d["edge_weight"] = ei[:, keep].contiguous(), ew[keep].contiguous()
    return d


def single_graph(seed):
    gen = torch.Generator().manual_seed(seed)
    ei, ew = G.er_graph(30, 0.15, gen, True)
    return dict(x=torch.randn(30, 4, generator=gen), edge_index=ei, edge_weight=ew, batch=None)


def tiny_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    x, ei, ew, batch = G.batched_graphs([6, 5, 5], 0.4, gen, 4, True)  # 16 nodes in all
    return dict(x=x, edge_index=ei, edge_weight=ew, batch=batch)


def main():
    for h, tag in ((None, "none"), ("greedy", "greedy"), ("w-greedy", "wgreedy")):
        for k in (1, 2, 3):
            add_case(f"kmis_linear_{tag}_k{k}", dict(in_channels=4, order_k=k, score_heuristic=h),
                     denser_batch if h == "w-greedy" else undirected_batch, 100 * k)
    add_case("kmis_directed_k2", dict(in_channels=4, order_k=2), directed_batch, 400)
    add_case("kmis_edgeless_isolated_k1", dict(in_channels=4, order_k=1), edgeless_batch, 500)
    add_case("kmis_single_graph_k2", dict(in_channels=4, order_k=2), single_graph, 600)
    add_case("kmis_reduce_none_k1", dict(in_channels=4, order_k=1, reduce_red_op=None), four_graphs, 700)
    add_case("kmis_degree_norm_k1", dict(in_channels=4, order_k=1, degree_norm=True), four_graphs, 800)
    add_case("kmis_edge_weight_norm_k2", dict(in_channels=4, order_k=2, edge_weight_norm=True), four_graphs, 820)
    add_case("kmis_keep_self_loops_k1", dict(in_channels=4, order_k=1, remove_self_loops=False), four_graphs, 840)
    add_case("kmis_canonical_none_k2", dict(order_k=2, scorer="canonical", score_heuristic=None), four_graphs, 900)
    add_case("kmis_constant_greedy_k1", dict(order_k=1, scorer="constant"), tiny_batch, 1000)
    add_case("kmis_degree_greedy_k1", dict(order_k=1, scorer="degree"), tiny_batch, 1000)
    out = os.path.join(HERE, "golden_kmis_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
