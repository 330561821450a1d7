#!/usr/bin/env python3
"""Generate the golden vectors of ASAP pooling (``tests/golden/golden_asap_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_sag.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs ``ASAPooling`` on small
seeded inputs.  The stand-in has no ``LEConv``; the plain-torch restatement of PyG's code defined here,

    out_i = lin3(x_i) + sum_{e: dst(e) = i} w_e (lin1(x_src(e)) - lin2(x_i)),

is assigned to ``tgp.poolers.asap.LEConv`` before a pooler is built.  The ``GNN=`` class of the last but one case is a
restated ``GraphConv`` with edge weights.

A top-k over float scores is only a contract when the scores are apart, so a case is kept only if
  (a) per graph, the lowest kept and the highest dropped score (after the activation) differ by at least 1e-4 -- ten
      times the project's fp32 tolerance: rounding on another device cannot move a node across --, and
  (b) the float64 run selects the same nodes, and
  (c) per graph, the kept scores are pairwise 1e-4 apart: the kept nodes become supernodes in descending score, and a
      saturating sigmoid brings scores within one rounding of each other more often than SAG's tanh did.
Seeds are walked until a case passes; the seed is stored.  Every case also stores a float64 run: alpha, x_new, the raw
fitness, ``so.weight``, pooled x and the gradients of ``sum(x_pool ** 2)`` with respect to ``x`` and every parameter.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_asap.py
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as G  # noqa: E402  (installs the PyG stand-in and imports the reference)
import tgp.poolers.asap as RA  # noqa: E402
import tgp.select.topk_select as RT  # noqa: E402
from make_golden_dmon import directed_graphs  # noqa: E402

CASES = {}
SEEN = {}  # what the reference's forward handed on: alpha, x_new, the raw fitness, the score its top-k saw
_topk, _softmax = RT.topk, RA.softmax


def _watched_topk(x, ratio, batch, min_score=None, *args, **kwargs):
    SEEN["score"] = x.detach().clone()
    return _topk(x, ratio, batch, min_score, *args, **kwargs)


def _watched_softmax(src, index=None, *args, **kwargs):
    out = _softmax(src, index, *args, **kwargs)
    SEEN["alpha"] = out.detach().clone()
    return out


RT.topk = _watched_topk
RA.softmax = _watched_softmax


class LEConv(torch.nn.Module):
    """PyG's LEConv as its code computes it: message (a_j - b_i) w_e, a = lin1(x), b = lin2(x), plus lin3(x)."""

    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__()
        self.lin1 = torch.nn.Linear(in_channels, out_channels, bias=bias)
        self.lin2 = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.lin3 = torch.nn.Linear(in_channels, out_channels, bias=bias)

    def reset_parameters(self):
        for lin in (self.lin1, self.lin2, self.lin3):
            lin.reset_parameters()

    def forward(self, x, edge_index, edge_weight=None):
        msg = self.lin1(x)[edge_index[0]] - self.lin2(x)[edge_index[1]]
        if edge_weight is not None:
            msg = msg * edge_weight.view(-1, 1)
        out = torch.zeros(x.size(0), msg.size(1), dtype=x.dtype).index_add_(0, edge_index[1], msg) + self.lin3(x)
        SEEN["x_new"], SEEN["fitness"] = x.detach().clone(), out.detach().view(-1).clone()
        return out


RA.LEConv = LEConv


class GraphConv(torch.nn.Module):
    """PyG's GraphConv with edge weights: lin_rel(sum_j w_ji x_j) + lin_root(x_i)."""

    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__()
        self.lin_rel = torch.nn.Linear(in_channels, out_channels, bias=bias)
        self.lin_root = torch.nn.Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_rel.reset_parameters()
        self.lin_root.reset_parameters()

    def forward(self, x, edge_index, edge_weight=None):
        msg = x[edge_index[0]]
        if edge_weight is not None:
            msg = msg * edge_weight.view(-1, 1)
        return self.lin_rel(torch.zeros_like(x).index_add_(0, edge_index[1], msg)) + self.lin_root(x)


GNNS = {None: None, "graphconv": GraphConv}


def build(gnn, cfg):
    return RA.ASAPooling(GNN=GNNS[gnn], **cfg)


def run(pooler, inputs, dtype=torch.float32, grad=False):
    """One forward of the reference; returns (output, x, what SEEN holds of it)."""
    SEEN.clear()
    x = inputs["x"].to(dtype)
    if grad:
        x = x.clone().requires_grad_(True)
    ew = inputs["edge_weight"]
    out = pooler(x=x, adj=inputs["edge_index"], edge_weight=None if ew is None else ew.to(dtype), batch=inputs["batch"])
    assert sorted(SEEN) == ["alpha", "fitness", "score", "x_new"], "the reference's forward attends and selects once"
    return out, x, dict(SEEN)


def selection_ok(pooler, inputs):
    """(a), (b), (c): False sends the caller to the next seed."""
    with torch.no_grad():
        out, _, seen = run(pooler, inputs)
        score = seen["score"]
        kept = torch.zeros(score.numel(), dtype=torch.bool)
        kept[out.so.node_index] = True
        batch = inputs["batch"] if inputs["batch"] is not None else torch.zeros(score.numel(), dtype=torch.long)
        for g in range(int(batch.max()) + 1):
            k, d = score[(batch == g) & kept], score[(batch == g) & ~kept]
            if k.numel() and d.numel() and float(k.min() - d.max()) < 1e-4:  # (a)
                return False
            if k.numel() > 1 and float(k.sort().values.diff().min()) < 1e-4:  # (c)
                return False
        out64, _, _ = run(copy.deepcopy(pooler).double(), inputs, torch.float64)
        return bool(torch.equal(out64.so.node_index, out.so.node_index))  # (b)


def f64_run(gnn, cfg, params, inputs):
    pooler = build(gnn, cfg).double().eval()
    pooler.load_state_dict({k: v.double() for k, v in params.items()})
    out, x, seen = run(pooler, inputs, torch.float64, grad=True)
    names = [n for n, _ in pooler.named_parameters()]
    leaves = [x] + [p for _, p in pooler.named_parameters()]
    g = torch.autograd.grad((out.x ** 2).sum(), leaves, allow_unused=True)
    return {"alpha": G.t(seen["alpha"]), "x_new": G.t(seen["x_new"]), "score": G.t(seen["fitness"]),
            "weight": G.t(out.so.weight), "x": G.t(out.x),
            "grads": {"x": G.t(g[0] if g[0] is not None else torch.zeros_like(x)),
                      "params": {n: G.t(gi if gi is not None else torch.zeros_like(p))
                                 for n, gi, p in zip(names, g[1:], leaves[1:])}}}


def add_case(name, gnn, cfg, make_inputs, first_seed):
    for seed in range(first_seed, first_seed + 400):
        inputs = make_inputs(seed)
        torch.manual_seed(seed)
        pooler = build(gnn, cfg).eval()
        if selection_ok(pooler, inputs):
            break
    else:
        raise RuntimeError(f"{name}: no seed gave a well-separated selection")
    with torch.no_grad():
        out, _, seen = run(pooler, inputs)
    params = G.params_of(pooler)
    exp = G.pool_dict(out)
    exp.update(alpha=G.t(seen["alpha"]), x_new=G.t(seen["x_new"]), score=G.t(seen["fitness"]))
    assert name not in CASES, name
    CASES[name] = {"kind": "pool", "seed": seed, "gnn": gnn, "inputs": {k: G.t(v) for k, v in inputs.items()},
                   "params": params, "cfg": cfg, "expected": exp, "f64": f64_run(gnn, cfg, params, inputs)}
    print(f"{name}: seed {seed}, N={inputs['x'].size(0)}, E={inputs['edge_index'].size(1)}, K={out.so.num_supernodes}")


def _sizes(gen):
    return torch.randint(8, 25, (4,), generator=gen).tolist()


def undirected_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    x, ei, _, batch = G.batched_graphs(_sizes(gen), 0.3, gen, 4, False)
    return dict(x=x, edge_index=ei, edge_weight=None, batch=batch)


def weighted_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    x, ei, ew, batch = G.batched_graphs(_sizes(gen), 0.3, gen, 4, True)
    return dict(x=x, edge_index=ei, edge_weight=ew, batch=batch)


def directed_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    x, ei, _, batch = directed_graphs(_sizes(gen), 0.2, gen, 4)
    return dict(x=x, edge_index=ei, edge_weight=None, batch=batch)


def single_graph(seed):
    gen = torch.Generator().manual_seed(seed)
    ei, _ = G.er_graph(24, 0.25, gen, False)
    return dict(x=torch.randn(24, 4, generator=gen), edge_index=ei, edge_weight=None, batch=None)


def self_loop_batch(seed):
    """The weighted batch with a weighted self-loop on every third node, then the whole list shuffled."""
    d = weighted_batch(seed)
    gen = torch.Generator().manual_seed(seed + 7)
    loops = torch.arange(0, d["x"].size(0), 3)
    ei = torch.cat([d["edge_index"], torch.stack([loops, loops])], 1)
    ew = torch.cat([d["edge_weight"], torch.rand(loops.numel(), generator=gen) + 0.1])
    order = torch.randperm(ei.size(1), generator=gen)
    d["edge_index"], d["edge_weight"] = ei[:, order].contiguous(), ew[order].contiguous()
    return d


def duplicate_batch(seed):
    """The directed batch with a third of its edges listed a second time, then the whole list shuffled."""
    d = directed_batch(seed)
    gen = torch.Generator().manual_seed(seed + 11)
    ei = d["edge_index"]
    again = torch.randperm(ei.size(1), generator=gen)[: ei.size(1) // 3]
    ei = torch.cat([ei, ei[:, again]], 1)
    d["edge_index"] = ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous()
    return d


def isolated_batch(seed):
    """The undirected batch without the edges of node 2 and of the last node: their only in-edge is the loop."""
    d = undirected_batch(seed)
    ei, last = d["edge_index"], d["x"].size(0) - 1
    keep = (ei[0] != 2) & (ei[1] != 2) & (ei[0] != last) & (ei[1] != last)
    d["edge_index"] = ei[:, keep].contiguous()
    return d


def one_column_batch(seed):
    d = weighted_batch(seed)
    d["x"] = d["x"][:, 0].contiguous()
    return d


def main():
    add_case("asap_undirected", None, dict(in_channels=4), undirected_batch, 100)
    add_case("asap_directed", None, dict(in_channels=4), directed_batch, 150)
    add_case("asap_single_graph", None, dict(in_channels=4), single_graph, 200)
    add_case("asap_weighted", None, dict(in_channels=4), weighted_batch, 250)
    add_case("asap_self_loops_unsorted", None, dict(in_channels=4), self_loop_batch, 300)
    add_case("asap_duplicates", None, dict(in_channels=4), duplicate_batch, 350)
    add_case("asap_isolated", None, dict(in_channels=4), isolated_batch, 400)
    add_case("asap_int_ratio", None, dict(in_channels=4, ratio=3), undirected_batch, 450)
    add_case("asap_tanh", None, dict(in_channels=4, nonlinearity="tanh"), weighted_batch, 500)
    add_case("asap_slope_zero", None, dict(in_channels=4, negative_slope=0.0), undirected_batch, 550)
    add_case("asap_keep_self_loops", None, dict(in_channels=4, remove_self_loops=False), self_loop_batch, 600)
    add_case("asap_degree_norm", None, dict(in_channels=4, degree_norm=True), weighted_batch, 650)
    add_case("asap_connect_max", None, dict(in_channels=4, connect_red_op="max"), duplicate_batch, 700)
    add_case("asap_gnn", "graphconv", dict(in_channels=4), weighted_batch, 750)
    add_case("asap_one_column", None, dict(in_channels=1), one_column_batch, 800)
    out = os.path.join(HERE, "golden_asap_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
