#!/usr/bin/env python3
"""Generate the golden vectors of edge-contraction pooling (``tests/golden/golden_edgepool_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_kmis.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs
``EdgeContractionPooling`` on small seeded inputs; no leaf is missing for this pooler.

The reference's tie order is not a contract (its ``argsort`` is not stable), so a case is kept only if
  (a) the reference's own ``argsort`` of its edge scores equals the stable one (``torch.argsort`` is wrapped inside the
      reference module, so it is the very call of the forward that is compared),
  (b) adjacent DISTINCT sorted scores differ by at least 1e-5 relative (the project's fp32 tolerance: rounding on another
      device cannot reorder such a case; exact ties, e.g. the targets with one incoming entry under softmax, are resolved
      by position on both sides), and
  (c) the order computed in float64 is the same.
Seeds are walked until a case passes; the seed is stored.  Every case also stores a float64 run: edge scores, weights,
pooled x and the gradients of ``sum(x_pool ** 2)`` with respect to ``x`` and the scorer's parameters.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_edgepool.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as G  # noqa: E402  (installs the PyG stand-in and imports the reference)
import tgp.select.edge_contraction_select as RE  # noqa: E402
from make_golden_dmon import directed_graphs  # noqa: E402
from tgp.poolers.edge_contraction import EdgeContractionPooling  # noqa: E402
from tgp.select import EdgeContractionSelect  # noqa: E402


class _TorchWithWatchedArgsort:
    """``torch`` as the reference module sees it, with ``argsort`` recording its argument and whether the order it
    returned is the stable one."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def argsort(self, e, *args, **kwargs):
        got = torch.argsort(e, *args, **kwargs)
        stable = torch.argsort(e, dim=0, descending=kwargs.get("descending", False), stable=True)
        self.calls.append((e.detach().clone(), bool(torch.equal(got, stable)), stable))
        return got


WATCH = _TorchWithWatchedArgsort()
RE.torch = WATCH

METHODS = {"softmax": EdgeContractionSelect.compute_edge_score_softmax,
           "tanh": EdgeContractionSelect.compute_edge_score_tanh,
           "sigmoid": EdgeContractionSelect.compute_edge_score_sigmoid}
CASES = {}


def build(cfg, method):
    return EdgeContractionPooling(edge_score_method=METHODS[method], **cfg)


def run(pooler, inputs, dtype=torch.float32, grad=False):
    """One forward of the reference; returns (output, the scores its argsort saw, was that order stable, stable order)."""
    WATCH.calls.clear()
    x = inputs["x"].to(dtype)
    if grad:
        x = x.clone().requires_grad_(True)
    ew = inputs["edge_weight"]
    out = pooler(x=x, adj=inputs["edge_index"], edge_weight=None if ew is None else ew.to(dtype), batch=inputs["batch"])
    assert len(WATCH.calls) == 1, "the reference's forward sorts its scores exactly once"
    e, was_stable, stable = WATCH.calls[0]
    return out, x, e, was_stable, stable


def order_ok(pooler, inputs):
    """(a), (b), (c): False sends the caller to the next seed."""
    import copy
    with torch.no_grad():
        _, _, e, was_stable, stable = run(pooler, inputs)
        if not was_stable:  # (a)
            return False
        s = e[stable]
        gap = (s[:-1] - s[1:]) / s[:-1].abs().clamp_min(1e-30)
        gap = gap[s[:-1] != s[1:]]
        if gap.numel() and float(gap.min()) < 1e-5:  # (b)
            return False
        _, _, e64, _, stable64 = run(copy.deepcopy(pooler).double(), inputs, torch.float64)
        return bool(torch.equal(stable64, stable))  # (c)


def f64_run(cfg, method, params, inputs):
    pooler = build(cfg, method).double().eval()
    pooler.load_state_dict({k: v.double() for k, v in params.items()})
    out, x, e, _, _ = run(pooler, inputs, torch.float64, grad=True)
    names = [n for n, _ in pooler.named_parameters()]
    leaves = [x] + [p for _, p in pooler.named_parameters()]
    g = torch.autograd.grad((out.x ** 2).sum(), leaves, allow_unused=True)
    return {"score": G.t(e), "weight": G.t(out.so.weight), "x": G.t(out.x),
            "grads": {"x": G.t(g[0] if g[0] is not None else torch.zeros_like(x)),
                      "params": {n: G.t(gi if gi is not None else torch.zeros_like(p))
                                 for n, gi, p in zip(names, g[1:], leaves[1:])}}}


def add_case(name, method, cfg, make_inputs, first_seed):
    for seed in range(first_seed, first_seed + 200):
        inputs = make_inputs(seed)
        torch.manual_seed(seed)
        pooler = build(cfg, method).eval()
        if order_ok(pooler, inputs):
            break
    else:
        raise RuntimeError(f"{name}: no seed gave a stable, well-separated order")
    with torch.no_grad():
        out, _, e, was_stable, _ = run(pooler, inputs)
    assert was_stable, "the reference's own order is not the stable one: not a usable case"
    params = G.params_of(pooler)
    exp = G.pool_dict(out)
    exp["score"] = G.t(e)
    del exp["so"]["node_index"]  # (0..N-1: the consumer rebuilds it)
    assert name not in CASES, name
    CASES[name] = {"kind": "pool", "seed": seed, "method": method, "inputs": {k: G.t(v) for k, v in inputs.items()},
                   "params": params, "cfg": cfg, "expected": exp, "f64": f64_run(cfg, method, params, inputs)}
    print(f"{name}: seed {seed}, N={inputs['x'].size(0)}, E={inputs['edge_index'].size(1)}, K={out.so.num_supernodes}")


def undirected_batch(seed, weighted=True):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(8, 25, (4,), generator=gen).tolist()
    x, ei, ew, batch = G.batched_graphs(sizes, 0.3, gen, 4, weighted)  # (dense enough that few targets have one entry)
    return dict(x=x, edge_index=ei, edge_weight=ew, batch=batch)


def unweighted_batch(seed):
    return undirected_batch(seed, weighted=False)


def directed_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(8, 25, (4,), generator=gen).tolist()
    x, ei, ew, batch = directed_graphs(sizes, 0.2, gen, 4)
    return dict(x=x, edge_index=ei, edge_weight=ew, batch=batch)


def single_graph(seed):
    gen = torch.Generator().manual_seed(seed)
    ei, ew = G.er_graph(32, 0.2, gen, True)
    return dict(x=torch.randn(32, 4, generator=gen), edge_index=ei, edge_weight=ew, batch=None)


def main():
    add_case("edgepool_softmax_batch", "softmax", dict(in_channels=4), undirected_batch, 100)
    add_case("edgepool_tanh_batch", "tanh", dict(in_channels=4), undirected_batch, 200)
    add_case("edgepool_sigmoid_batch", "sigmoid", dict(in_channels=4, add_to_edge_score=0.0), undirected_batch, 300)
    add_case("edgepool_softmax_single_graph", "softmax", dict(in_channels=4), single_graph, 400)
    add_case("edgepool_tanh_single_graph", "tanh", dict(in_channels=4), single_graph, 450)
    add_case("edgepool_softmax_unweighted", "softmax", dict(in_channels=4), unweighted_batch, 500)
    add_case("edgepool_sigmoid_unweighted", "sigmoid", dict(in_channels=4), unweighted_batch, 550)
    add_case("edgepool_softmax_connect_max", "softmax", dict(in_channels=4, connect_red_op="max"), undirected_batch, 600)
    add_case("edgepool_tanh_connect_max", "tanh", dict(in_channels=4, connect_red_op="max"), undirected_batch, 650)
    add_case("edgepool_sigmoid_degree_norm", "sigmoid", dict(in_channels=4, degree_norm=True), undirected_batch, 700)
    add_case("edgepool_softmax_degree_norm", "softmax", dict(in_channels=4, degree_norm=True), undirected_batch, 750)
    add_case("edgepool_softmax_directed", "softmax", dict(in_channels=4), directed_batch, 800)
    add_case("edgepool_tanh_directed", "tanh", dict(in_channels=4, add_to_edge_score=0.0), directed_batch, 850)
    add_case("edgepool_softmax_keep_self_loops", "softmax", dict(in_channels=4, remove_self_loops=False), undirected_batch,
             900)
    out = os.path.join(HERE, "golden_edgepool_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
