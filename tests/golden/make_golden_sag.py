#!/usr/bin/env python3
"""Generate the golden vectors of self-attention graph pooling (``tests/golden/golden_sag_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_edgepool.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs ``SAGPooling`` on
small seeded inputs.  The stand-in has no graph convolutions, so the ``GNN=`` classes handed to the reference are
plain-torch restatements of PyG's ``GraphConv`` and ``SAGEConv`` (gather, ``index_add_``, two ``Linear``s, PyG's
parameter names) defined here.

A top-k over float scores is only a contract when the scores are apart, so a case is kept only if
  (a) per graph, the lowest kept and the highest dropped score (after the activation / the softmax) differ by at least
      1e-4 -- ten times the project's fp32 tolerance: rounding on another device cannot move a node across --, in
      ``min_score`` mode no score lies within 1e-5 of the threshold, and
  (b) the float64 run selects the same nodes.
Seeds are walked until a case passes; the seed is stored.  Every case also stores a float64 run: the raw score,
``so.weight``, pooled x and the gradients of ``sum(x_pool ** 2)`` with respect to ``x`` and every parameter.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sag.py
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as G  # noqa: E402  (installs the PyG stand-in and imports the reference)
import tgp.select.topk_select as RT  # noqa: E402
from make_golden_dmon import directed_graphs  # noqa: E402
from tgp.poolers.sag import SAGPooling  # noqa: E402

CASES = {}
SEEN = []  # the scores the reference's top-k saw, one entry per forward
_topk = RT.topk


def _watched_topk(x, ratio, batch, min_score=None, *args, **kwargs):
    SEEN.append(x.detach().clone())
    return _topk(x, ratio, batch, min_score, *args, **kwargs)


RT.topk = _watched_topk


def _aggregate(x, edge_index, mean):
    out = torch.zeros_like(x).index_add_(0, edge_index[1], x[edge_index[0]])
    if mean:
        deg = torch.zeros(x.size(0), dtype=x.dtype).index_add_(0, edge_index[1], torch.ones(edge_index.size(1), dtype=x.dtype))
        out = out / deg.clamp(min=1).view(-1, 1)
    return out


class GraphConv(torch.nn.Module):
    """PyG's GraphConv without edge weights: lin_rel(aggr_j x_j) + lin_root(x_i)."""

    def __init__(self, in_channels, out_channels, aggr="add", bias=True):
        super().__init__()
        self.aggr = aggr
        self.lin_rel = torch.nn.Linear(in_channels, out_channels, bias=bias)
        self.lin_root = torch.nn.Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_rel.reset_parameters()
        self.lin_root.reset_parameters()

    def forward(self, x, edge_index, edge_weight=None):
        return self.lin_rel(_aggregate(x, edge_index, self.aggr == "mean")) + self.lin_root(x)


class SAGEConv(torch.nn.Module):
    """PyG's SAGEConv: lin_l(mean_j x_j) + lin_r(x_i)."""

    def __init__(self, in_channels, out_channels, aggr="mean", root_weight=True, bias=True):
        super().__init__()
        self.aggr, self.root_weight = aggr, root_weight
        self.lin_l = torch.nn.Linear(in_channels, out_channels, bias=bias)
        if root_weight:
            self.lin_r = torch.nn.Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        if self.root_weight:
            self.lin_r.reset_parameters()

    def forward(self, x, edge_index):
        out = self.lin_l(_aggregate(x, edge_index, self.aggr == "mean"))
        return out + self.lin_r(x) if self.root_weight else out


GNNS = {"graphconv": GraphConv, "sage": SAGEConv}


def build(gnn, cfg):
    return SAGPooling(GNN=GNNS[gnn], **cfg)


def run(pooler, inputs, dtype=torch.float32, grad=False):
    """One forward of the reference; returns (output, x, the raw score of the GNN, the score its top-k saw)."""
    SEEN.clear()
    x = inputs["x"].to(dtype)
    if grad:
        x = x.clone().requires_grad_(True)
    ew, attn = inputs["edge_weight"], inputs.get("attn")
    out = pooler(x=x, adj=inputs["edge_index"], edge_weight=None if ew is None else ew.to(dtype), batch=inputs["batch"],
                 attn=None if attn is None else attn.to(dtype))
    assert len(SEEN) == 1, "the reference's forward selects exactly once"
    a = x if attn is None else attn.to(dtype)
    with torch.no_grad():
        raw = pooler.gnn(a.detach().view(-1, 1) if a.dim() == 1 else a.detach(), inputs["edge_index"]).view(-1)
    return out, x, raw, SEEN[0]


def selection_ok(pooler, inputs):
    """(a), (b): False sends the caller to the next seed."""
    with torch.no_grad():
        out, _, _, score = run(pooler, inputs)
        kept = torch.zeros(score.numel(), dtype=torch.bool)
        kept[out.so.node_index] = True
        batch = inputs["batch"] if inputs["batch"] is not None else torch.zeros(score.numel(), dtype=torch.long)
        for g in range(int(batch.max()) + 1):
            k, d = score[(batch == g) & kept], score[(batch == g) & ~kept]
            if k.numel() and d.numel() and float(k.min() - d.max()) < 1e-4:  # (a)
                return False
        ms = pooler.selector.min_score
        if ms is not None and float((score - ms).abs().min()) < 1e-5:
            return False
        out64, _, _, _ = run(copy.deepcopy(pooler).double(), inputs, torch.float64)
        return bool(torch.equal(out64.so.node_index, out.so.node_index))  # (b)


def f64_run(gnn, cfg, params, inputs):
    pooler = build(gnn, cfg).double().eval()
    pooler.load_state_dict({k: v.double() for k, v in params.items()})
    out, x, raw, _ = run(pooler, inputs, torch.float64, grad=True)
    names = [n for n, _ in pooler.named_parameters()]
    leaves = [x] + [p for _, p in pooler.named_parameters()]
    g = torch.autograd.grad((out.x ** 2).sum(), leaves, allow_unused=True)
    return {"score": G.t(raw), "weight": G.t(out.so.weight), "x": G.t(out.x),
            "grads": {"x": G.t(g[0] if g[0] is not None else torch.zeros_like(x)),
                      "params": {n: G.t(gi if gi is not None else torch.zeros_like(p))
                                 for n, gi, p in zip(names, g[1:], leaves[1:])}}}


def add_case(name, gnn, cfg, make_inputs, first_seed):
    for seed in range(first_seed, first_seed + 200):
        inputs = make_inputs(seed)
        torch.manual_seed(seed)
        pooler = build(gnn, cfg).eval()
        if selection_ok(pooler, inputs):
            break
    else:
        raise RuntimeError(f"{name}: no seed gave a well-separated selection")
    with torch.no_grad():
        out, _, raw, _ = run(pooler, inputs)
    params = G.params_of(pooler)
    exp = G.pool_dict(out)
    exp["score"] = G.t(raw)
    assert name not in CASES, name
    CASES[name] = {"kind": "pool", "seed": seed, "gnn": gnn, "inputs": {k: G.t(v) for k, v in inputs.items()},
                   "params": params, "cfg": cfg, "expected": exp, "f64": f64_run(gnn, cfg, params, inputs)}
    print(f"{name}: seed {seed}, N={inputs['x'].size(0)}, E={inputs['edge_index'].size(1)}, K={out.so.num_supernodes}")


def undirected_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(8, 25, (4,), generator=gen).tolist()
    x, ei, ew, batch = G.batched_graphs(sizes, 0.3, gen, 4, True)
    return dict(x=x, edge_index=ei, edge_weight=ew, batch=batch)


def directed_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(8, 25, (4,), generator=gen).tolist()
    x, ei, ew, batch = directed_graphs(sizes, 0.2, gen, 4)
    return dict(x=x, edge_index=ei, edge_weight=ew, batch=batch)


def single_graph(seed):
    gen = torch.Generator().manual_seed(seed)
    ei, ew = G.er_graph(32, 0.2, gen, True)
    return dict(x=torch.randn(32, 4, generator=gen), edge_index=ei, edge_weight=ew, batch=None)


def self_loop_batch(seed):
    """The undirected batch with a self-loop on every third node appended: the list is no longer sorted."""
    d = undirected_batch(seed)
    gen = torch.Generator().manual_seed(seed + 7)
    loops = torch.arange(0, d["x"].size(0), 3)
    d["edge_index"] = torch.cat([d["edge_index"], torch.stack([loops, loops])], 1)
    d["edge_weight"] = torch.cat([d["edge_weight"], torch.rand(loops.numel(), generator=gen) + 0.1])
    return d


def attn_2d_batch(seed):
    d = undirected_batch(seed)
    d["attn"] = torch.randn(d["x"].size(0), 3, generator=torch.Generator().manual_seed(seed + 11))
    return d


def attn_1d_batch(seed):
    d = undirected_batch(seed)
    d["attn"] = torch.randn(d["x"].size(0), generator=torch.Generator().manual_seed(seed + 13))
    return d


def main():
    add_case("sag_graphconv_batch", "graphconv", dict(in_channels=4), undirected_batch, 100)
    add_case("sag_graphconv_single_graph", "graphconv", dict(in_channels=4), single_graph, 150)
    add_case("sag_graphconv_directed", "graphconv", dict(in_channels=4), directed_batch, 200)
    add_case("sag_graphconv_mean", "graphconv", dict(in_channels=4, aggr="mean"), undirected_batch, 250)
    add_case("sag_sage_batch", "sage", dict(in_channels=4), undirected_batch, 300)
    add_case("sag_sage_directed", "sage", dict(in_channels=4), directed_batch, 350)
    add_case("sag_int_ratio", "graphconv", dict(in_channels=4, ratio=3), undirected_batch, 400)
    add_case("sag_min_score", "graphconv", dict(in_channels=4, min_score=0.05), undirected_batch, 450)
    add_case("sag_multiplier", "graphconv", dict(in_channels=4, multiplier=2.0), undirected_batch, 500)
    add_case("sag_attn_2d", "graphconv", dict(in_channels=3), attn_2d_batch, 550)
    add_case("sag_attn_1d", "graphconv", dict(in_channels=1), attn_1d_batch, 600)
    add_case("sag_identity", "graphconv", dict(in_channels=4, nonlinearity="identity"), undirected_batch, 650)
    add_case("sag_keep_self_loops", "graphconv", dict(in_channels=4, remove_self_loops=False), self_loop_batch, 700)
    add_case("sag_degree_norm", "graphconv", dict(in_channels=4, degree_norm=True), undirected_batch, 750)
    add_case("sag_connect_max", "sage", dict(in_channels=4, connect_red_op="max"), undirected_batch, 800)
    out = os.path.join(HERE, "golden_sag_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
