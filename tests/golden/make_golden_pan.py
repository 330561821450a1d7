#!/usr/bin/env python3
"""Generate the golden vectors of PAN pooling (``tests/golden/golden_pan_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_sag.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs ``PANPooling`` on small
seeded inputs.  The stand-in has no ``PANConv``, so the MET matrix the reference is fed comes from
``tests/pan_restatement.py`` (``x_in -> conv -> (x, M)``); the pooler's own code -- score, ``TopkSelect``, ``BaseReduce``,
``SparseConnect`` -- is the reference's.

How the reference was driven: its ``forward`` itself.  The module asserts ``HAS_TORCH_SPARSE`` in the constructor and
calls ``adj.coo()``; the flag is patched in its module for the time of the construction and ``M`` is a coalesced torch
COO tensor that carries a ``coo()`` attribute returning ``(row, col, values)``.  Nothing of the forward was replaced.

The separated-scores rule of the SAG generator is kept: a case is stored only if (a) per graph the lowest kept and the
highest dropped score differ by at least 1e-4 (in ``min_score`` mode no score lies within 1e-5 of the threshold) and
(b) the float64 run selects the same nodes.  Seeds are walked until a case passes; the seed is stored.  Every case also
stores a float64 run with the gradients of ``sum(x_pool ** 2)`` with respect to the convolution's input and every
parameter of the convolution and the pooler.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pan.py
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import make_golden as G  # noqa: E402  (installs the PyG stand-in and imports the reference)
import tgp.poolers.pan as RP  # noqa: E402
import tgp.select.topk_select as RT  # noqa: E402
from make_golden_dmon import directed_graphs  # noqa: E402

import pan_restatement as R  # noqa: E402

CASES = {}
SEEN = []  # the scores the reference's top-k saw, one entry per forward
_topk = RT.topk


def _watched_topk(x, ratio, batch, min_score=None, *args, **kwargs):
    SEEN.append(x.detach().clone())
    return _topk(x, ratio, batch, min_score, *args, **kwargs)


RT.topk = _watched_topk


def build(cfg):
    RP.HAS_TORCH_SPARSE = True  # (the constructor's assert; nothing of torch_sparse is used with a torch COO input)
    try:
        return RP.PANPooling(**cfg)
    finally:
        RP.HAS_TORCH_SPARSE = False


def met_tensor(index, values, n):
    m = torch.sparse_coo_tensor(index, values, (n, n), is_coalesced=True)
    m.coo = lambda: (index[0], index[1], values)
    return m


def run(pooler, conv, inputs, dtype=torch.float32, grad=False):
    """One forward: the restated convolution, then the reference's pooler.  Returns (output, leaves of the convolution
    (x_in, weight, lin_w, lin_b), the convolution's output, M's index and values, the score the top-k saw)."""
    SEEN.clear()
    leaves = [inputs["x"].to(dtype)] + [conv[k].to(dtype) for k in ("weight", "lin.weight", "lin.bias")]
    if grad:
        leaves = [v.clone().requires_grad_(True) for v in leaves]
    x_in, w, lin_w, lin_b = leaves
    x, index, values = R.conv(x_in, inputs["edge_index"], w, lin_w, lin_b, inputs["batch"])
    out = pooler(x=x, adj=met_tensor(index, values, x.size(0)), batch=inputs["batch"])
    assert len(SEEN) == 1, "the reference's forward selects exactly once"
    return out, leaves, x, index, values, SEEN[0]


def selection_ok(pooler, conv, inputs):
    with torch.no_grad():
        out, _, _, _, _, score = run(pooler, conv, inputs)
        score = score.view(-1)
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
        out64, _, _, _, _, _ = run(copy.deepcopy(pooler).double(), conv, inputs, torch.float64)
        return bool(torch.equal(out64.so.node_index, out.so.node_index))  # (b)


def f64_run(cfg, params, conv, inputs):
    pooler = build(cfg).double().eval()
    pooler.load_state_dict({k: v.double() for k, v in params.items()})
    out, leaves, x, _, values, _ = run(pooler, conv, inputs, torch.float64, grad=True)
    names = [n for n, _ in pooler.named_parameters()]
    every = leaves + [p for _, p in pooler.named_parameters()]
    g = torch.autograd.grad((out.x ** 2).sum(), every, allow_unused=True)
    g = [gi if gi is not None else torch.zeros_like(v) for gi, v in zip(g, every)]
    return {"conv_out": G.t(x), "met_values": G.t(values), "weight": G.t(out.so.weight), "x": G.t(out.x),
            "grads": {"x": G.t(g[0]), "conv": {"weight": G.t(g[1]), "lin.weight": G.t(g[2]), "lin.bias": G.t(g[3])},
                      "params": {n: G.t(gi) for n, gi in zip(names, g[4:])}}}


def add_case(name, cfg, make_inputs, first_seed, filter_size=2, out_channels=4):
    for seed in range(first_seed, first_seed + 200):
        inputs = make_inputs(seed)
        gen = torch.Generator().manual_seed(seed + 1)
        f_in = inputs["x"].size(1)
        conv = {"weight": torch.rand(filter_size + 1, generator=gen) * 0.8 + 0.2,
                "lin.weight": torch.randn(out_channels, f_in, generator=gen) / f_in ** 0.5,
                "lin.bias": torch.randn(out_channels, generator=gen) * 0.1}
        torch.manual_seed(seed)
        pooler = build(dict(in_channels=out_channels, **cfg)).eval()
        with torch.no_grad():  # the reset values (p = 1, beta = 0.5) moved, so that every parameter matters
            pooler.p.copy_(torch.rand(out_channels, generator=gen) + 0.5)
            pooler.beta.copy_(torch.rand(2, generator=gen) + 0.25)
        if selection_ok(pooler, conv, inputs):
            break
    else:
        raise RuntimeError(f"{name}: no seed gave a well-separated selection")
    with torch.no_grad():
        out, _, x, index, values, score = run(pooler, conv, inputs)
    params = G.params_of(pooler)
    exp = G.pool_dict(out)
    exp.update(score=G.t(score.view(-1)), conv_out=G.t(x), met_index=G.t(index), met_values=G.t(values))
    assert name not in CASES, name
    full = dict(in_channels=out_channels, **cfg)
    CASES[name] = {"kind": "pool", "seed": seed, "filter_size": filter_size, "inputs": {k: G.t(v) for k, v in inputs.items()},
                   "conv": {k: G.t(v) for k, v in conv.items()}, "params": params, "cfg": full, "expected": exp,
                   "f64": f64_run(full, params, conv, inputs)}
    print(f"{name}: seed {seed}, N={inputs['x'].size(0)}, E={inputs['edge_index'].size(1)}, nnz={index.size(1)}, "
          f"K={out.so.num_supernodes}")


def undirected_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(8, 25, (4,), generator=gen).tolist()
    x, ei, _, batch = G.batched_graphs(sizes, 0.2, gen, 3, True)
    return dict(x=x, edge_index=ei, batch=batch)


def directed_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(8, 25, (4,), generator=gen).tolist()
    x, ei, _, batch = directed_graphs(sizes, 0.15, gen, 3)
    return dict(x=x, edge_index=ei, batch=batch)


def single_graph(seed):
    gen = torch.Generator().manual_seed(seed)
    ei, _ = G.er_graph(30, 0.12, gen, False)
    return dict(x=torch.randn(30, 3, generator=gen), edge_index=ei, batch=None)


def loops_and_duplicates(seed):
    """The undirected batch with a self-loop on every third node and every fifth edge listed twice, appended: the list
    is no longer sorted."""
    d = undirected_batch(seed)
    loops = torch.arange(0, d["x"].size(0), 3)
    d["edge_index"] = torch.cat([d["edge_index"], torch.stack([loops, loops]), d["edge_index"][:, ::5]], 1)
    return d


def with_edgeless_graph(seed):
    """Four graphs, the third without edges."""
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(6, 16, (4,), generator=gen).tolist()
    x, ei, _, batch = G.batched_graphs(sizes, 0.25, gen, 3, True)
    lo = sum(sizes[:2])
    keep = ~((ei[0] >= lo) & (ei[0] < lo + sizes[2]))
    return dict(x=x, edge_index=ei[:, keep].contiguous(), batch=batch)


def main():
    add_case("pan_undirected_batch", {}, undirected_batch, 100)
    add_case("pan_directed_batch", {}, directed_batch, 150)
    add_case("pan_single_graph", {}, single_graph, 200)
    add_case("pan_loops_and_duplicates", {}, loops_and_duplicates, 250)
    add_case("pan_edgeless_graph", {}, with_edgeless_graph, 300)
    add_case("pan_min_score", dict(min_score=0.05), undirected_batch, 350)
    add_case("pan_int_ratio", dict(ratio=3), undirected_batch, 400)
    add_case("pan_multiplier", dict(multiplier=2.0), undirected_batch, 450)
    add_case("pan_degree_norm", dict(degree_norm=True), undirected_batch, 500)
    add_case("pan_connect_max", dict(connect_red_op="max"), undirected_batch, 550)
    add_case("pan_identity", dict(nonlinearity="identity"), undirected_batch, 600)
    for L in (1, 3, 4):
        add_case(f"pan_filter_{L}", {}, directed_batch, 650 + 50 * L, filter_size=L)
    out = os.path.join(HERE, "golden_pan_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
