#!/usr/bin/env python3
"""Generate the golden vectors of MaxCut pooling (``tests/golden/golden_maxcut_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_asap.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs ``MaxCutPooling`` on
small seeded inputs.  The stand-in has no ``GCNConv`` and no ``Linear``; the plain-torch restatement of
``GCNConv(normalize=False)`` defined here,

    out_i = sum_{e: dst(e) = i} w_e (W x_src(e)) + b,

and ``torch.nn.Linear`` are assigned into ``tgp.select.maxcut_select`` before a pooler is built.  Biases are drawn at
random after construction (PyG's start at zero, which would leave the bias add untested).

A top-k over float scores is only a contract when the scores are apart, so a case is kept only if
  (a) per graph, the lowest kept and the highest dropped score differ by at least 1e-4 -- ten times the project's fp32
      tolerance: rounding on another device cannot move a node across --, and
  (b) the float64 run (with explicit float64 edge weights: the reference's Laplacian makes float32 ones otherwise)
      selects the same nodes, and
  (c) per graph, the kept scores are pairwise 1e-4 apart, and
  (d) no node is left to the random draw of ``get_random_map_mask``.
Seeds are walked until a case passes; the seed is stored.  Every case stores the scores, the kept nodes, the pooled
output with its ``SelectOutput`` and loss, and a float64 run: the same outputs and the gradients of
``sum(x_pool ** 2) + loss`` with respect to ``x`` and every parameter.  Two extra cases store less: the empty edge list
(every score is the same number, so nothing about its selection is a contract) stores its scores and loss, and a path
longer than ``max_iter`` has leftovers on purpose and stores its inputs, scores and the kept set.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_maxcut.py
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as G  # noqa: E402  (installs the PyG stand-in and imports the reference)
import tgp.poolers.maxcut as RP  # noqa: E402
import tgp.select.maxcut_select as RM  # noqa: E402
import tgp.select.topk_select as RT  # noqa: E402
import tgp.utils.ops as RO  # noqa: E402
from make_golden_dmon import directed_graphs  # noqa: E402

CASES = {}
SEEN = {}  # what the reference's forward handed on: the score its top-k saw, the nodes it kept, a random draw
_topk, _random_map = RT.topk, RO.get_random_map_mask


def _watched_topk(x, ratio, batch, min_score=None, *args, **kwargs):
    out = _topk(x, ratio, batch, min_score, *args, **kwargs)
    SEEN["score"], SEEN["kept"] = x.detach().clone(), out.detach().clone()
    return out


def _watched_random_map(*args, **kwargs):
    SEEN["random"] = True
    return _random_map(*args, **kwargs)


RT.topk = _watched_topk
RO.get_random_map_mask = _watched_random_map


class GCNConv(torch.nn.Module):
    """PyG's GCNConv with ``normalize=False`` as its code computes it: project, weight the messages, add, add the bias."""

    def __init__(self, in_channels, out_channels, normalize=False, cached=False):
        super().__init__()
        assert not normalize
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.lin.weight)
        torch.nn.init.zeros_(self.bias)

    def forward(self, x, edge_index, edge_weight=None):
        z = self.lin(x)
        msg = z[edge_index[0]]
        if edge_weight is not None:
            msg = msg * edge_weight.view(-1, 1)
        return torch.zeros_like(z).index_add_(0, edge_index[1], msg) + self.bias


RM.GCNConv = GCNConv
RM.Linear = torch.nn.Linear

SMALL = dict(in_channels=4, mp_units=[8, 8], mlp_units=[4])


def build(cfg, seed):
    torch.manual_seed(seed)
    pooler = RP.MaxCutPooling(**cfg).eval()
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in pooler.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.rand(p.shape, generator=gen) - 0.5)
    return pooler


def run(pooler, inputs, dtype=torch.float32, grad=False):
    """One forward of the reference; returns (output, x, what SEEN holds of it)."""
    SEEN.clear()
    x = inputs["x"].to(dtype)
    if grad:
        x = x.clone().requires_grad_(True)
    ew = inputs["edge_weight"]
    if dtype == torch.float64:  # explicit float64 weights (the reference's own ones would be float32)
        ew = torch.ones(inputs["edge_index"].size(1), dtype=dtype) if ew is None else ew.to(dtype)
    out = pooler(x=x, adj=inputs["edge_index"], edge_weight=ew, batch=inputs["batch"])
    assert "score" in SEEN and "kept" in SEEN, "the reference's forward selects once"
    return out, x, dict(SEEN)


def selection_ok(pooler, inputs, allow_random=False):
    """(a) .. (d): False sends the caller to the next seed."""
    with torch.no_grad():
        out, _, seen = run(pooler, inputs)
        if seen.get("random") and not allow_random:  # (d)
            return False
        score = seen["score"].view(-1)
        kept = torch.zeros(score.numel(), dtype=torch.bool)
        kept[seen["kept"]] = True
        batch = inputs["batch"] if inputs["batch"] is not None else torch.zeros(score.numel(), dtype=torch.long)
        for g in range(int(batch.max()) + 1):
            k, d = score[(batch == g) & kept], score[(batch == g) & ~kept]
            if k.numel() and d.numel() and float(k.min() - d.max()) < 1e-4:  # (a)
                return False
            if k.numel() > 1 and float(k.sort().values.diff().min()) < 1e-4:  # (c)
                return False
        _, _, seen64 = run(copy.deepcopy(pooler).double(), inputs, torch.float64)
        return bool(torch.equal(seen64["kept"], seen["kept"]))  # (b)


def expected_of(out, seen):
    exp = G.pool_dict(out)
    exp.update(scores=G.t(out.so.scores), kept=G.t(seen["kept"]), cluster_index=G.t(out.so.cluster_index))
    return exp


def f64_run(cfg, params, inputs):
    pooler = RP.MaxCutPooling(**cfg).double().eval()
    pooler.load_state_dict({k: v.double() for k, v in params.items()})
    out, x, seen = run(pooler, inputs, torch.float64, grad=True)
    names = [n for n, _ in pooler.named_parameters()]
    leaves = [x] + [p for _, p in pooler.named_parameters()]
    g = torch.autograd.grad((out.x ** 2).sum() + out.loss["maxcut_loss"], leaves, allow_unused=True)
    exp = expected_of(out, seen)
    # the parameter gradients as ONE vector in named_parameters() order (a tensor per parameter costs the file more in
    # per-record overhead than in numbers)
    flat = torch.cat([(gi if gi is not None else torch.zeros_like(p)).reshape(-1) for gi, p in zip(g[1:], leaves[1:])])
    exp["grads"] = {"x": G.t(g[0] if g[0] is not None else torch.zeros_like(x)), "names": names, "params_flat": G.t(flat)}
    return exp


def add_case(name, cfg, make_inputs, first_seed, allow_random=False):
    for seed in range(first_seed, first_seed + 400):
        inputs = make_inputs(seed)
        pooler = build(cfg, seed)
        if selection_ok(pooler, inputs, allow_random):
            break
    else:
        raise RuntimeError(f"{name}: no seed gave a well-separated selection without a random draw")
    with torch.no_grad():
        out, _, seen = run(pooler, inputs)
    params = G.params_of(pooler)
    assert name not in CASES, name
    CASES[name] = {"kind": "pool", "seed": seed, "inputs": {k: G.t(v) for k, v in inputs.items()}, "params": params,
                   "cfg": cfg, "expected": expected_of(out, seen), "f64": f64_run(cfg, params, inputs)}
    print(f"{name}: seed {seed}, N={inputs['x'].size(0)}, E={inputs['edge_index'].size(1)}, K={out.so.num_supernodes}")


def _sizes(gen):
    return torch.randint(6, 15, (3,), generator=gen).tolist()


def undirected_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    x, ei, _, batch = G.batched_graphs(_sizes(gen), 0.35, gen, 4, False)
    return dict(x=x, edge_index=ei, edge_weight=None, batch=batch)


def weighted_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    x, ei, ew, batch = G.batched_graphs(_sizes(gen), 0.35, gen, 4, True)
    return dict(x=x, edge_index=ei, edge_weight=ew, batch=batch)


def directed_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    x, ei, _, batch = directed_graphs(_sizes(gen), 0.25, gen, 4)
    return dict(x=x, edge_index=ei, edge_weight=None, batch=batch)


def directed_weighted_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    x, ei, ew, batch = directed_graphs(_sizes(gen), 0.25, gen, 4)
    return dict(x=x, edge_index=ei, edge_weight=ew, batch=batch)


def single_graph(seed):
    gen = torch.Generator().manual_seed(seed)
    ei, _ = G.er_graph(20, 0.25, gen, False)
    return dict(x=torch.randn(20, 4, generator=gen), edge_index=ei, edge_weight=None, batch=None)


def loops_and_duplicates(seed):
    """The weighted batch with a weighted self-loop on every third node and a third of its edges listed a second time
    (with weights of their own), then the whole list shuffled."""
    d = weighted_batch(seed)
    gen = torch.Generator().manual_seed(seed + 7)
    ei, ew = d["edge_index"], d["edge_weight"]
    loops = torch.arange(0, d["x"].size(0), 3)
    again = torch.randperm(ei.size(1), generator=gen)[: ei.size(1) // 3]
    ei = torch.cat([ei, torch.stack([loops, loops]), ei[:, again]], 1)
    ew = torch.cat([ew, torch.rand(loops.numel(), generator=gen) + 0.1, torch.rand(again.numel(), generator=gen) + 0.1])
    order = torch.randperm(ei.size(1), generator=gen)
    d["edge_index"], d["edge_weight"] = ei[:, order].contiguous(), ew[order].contiguous()
    return d


def isolated_batch(seed):
    """The undirected batch without the edges of node 2 and of the last node: node 2 keeps its diagonal term, the last
    node lies above every endpoint of the list and gets none.  (Both must be kept for the case to pass (d).)"""
    d = undirected_batch(seed)
    ei, last = d["edge_index"], d["x"].size(0) - 1
    keep = (ei[0] != 2) & (ei[1] != 2) & (ei[0] != last) & (ei[1] != last)
    d["edge_index"] = ei[:, keep].contiguous()
    return d


def empty_batch(seed):
    d = undirected_batch(seed)
    d["edge_index"] = torch.zeros(2, 0, dtype=torch.long)
    return d


def path_graph(seed):
    """Two paths of 16 nodes: with a kept node near one end the far end is more than ``max_iter`` hops away."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.arange(15)
    one = torch.cat([torch.stack([a, a + 1]), torch.stack([a + 1, a])], 1)
    ei = torch.cat([one, one + 16], 1)
    batch = torch.arange(2).repeat_interleave(16)
    return dict(x=torch.randn(32, 4, generator=gen), edge_index=ei, edge_weight=None, batch=batch)


def add_leftover_case(name, cfg, first_seed):
    """A case whose assignment needs the random draw: inputs, parameters and the kept set only."""
    for seed in range(first_seed, first_seed + 400):
        inputs = path_graph(seed)
        pooler = build(cfg, seed)
        with torch.no_grad():
            out, _, seen = run(pooler, inputs)
        if seen.get("random") and selection_ok(pooler, inputs, True):
            break
    else:
        raise RuntimeError(f"{name}: no seed left a node to the random draw")
    CASES[name] = {"kind": "leftover", "seed": seed, "inputs": {k: G.t(v) for k, v in inputs.items()},
                   "params": G.params_of(pooler), "cfg": cfg, "expected": {"kept": G.t(seen["kept"]),
                                                                           "scores": G.t(out.so.scores)}}
    print(f"{name}: seed {seed}, kept {seen['kept'].tolist()}")


def add_scores_case(name, cfg, make_inputs, seed):
    """A case whose scores are all equal (no edges: every layer gives act(b)), so its selection is no contract: the
    scores and the loss only, in float32 and float64."""
    inputs = make_inputs(seed)
    pooler = build(cfg, seed)
    with torch.no_grad():
        out, _, _ = run(pooler, inputs)
        out64, _, _ = run(copy.deepcopy(pooler).double(), inputs, torch.float64)
    CASES[name] = {"kind": "scores", "seed": seed, "inputs": {k: G.t(v) for k, v in inputs.items()},
                   "params": G.params_of(pooler), "cfg": cfg,
                   "expected": {"scores": G.t(out.so.scores), "loss": {k: G.t(v) for k, v in out.loss.items()}},
                   "f64": {"scores": G.t(out64.so.scores), "loss": {k: G.t(v) for k, v in out64.loss.items()}}}
    print(f"{name}: seed {seed}, N={inputs['x'].size(0)}, E=0")


def main():
    add_case("maxcut_default", dict(in_channels=4), undirected_batch, 100)
    # (no batch vector: the reference's Connect refuses edge_weight_norm without the pooled batch)
    add_case("maxcut_single_graph", dict(SMALL, edge_weight_norm=False), single_graph, 150)
    add_case("maxcut_directed", dict(SMALL), directed_batch, 200)
    add_case("maxcut_weighted", dict(SMALL), weighted_batch, 250)
    add_case("maxcut_directed_weighted", dict(SMALL), directed_weighted_batch, 300)
    add_case("maxcut_loops_duplicates", dict(SMALL), loops_and_duplicates, 350)
    add_case("maxcut_isolated", dict(SMALL), isolated_batch, 400)
    add_scores_case("maxcut_empty", dict(SMALL, assign_all_nodes=False), empty_batch, 450)
    add_case("maxcut_no_assign_all", dict(SMALL, assign_all_nodes=False), undirected_batch, 500)
    add_case("maxcut_12_layers", dict(in_channels=4, mp_units=[8, 8, 8, 8, 6, 6, 6, 6, 4, 4, 4, 4], mlp_units=[4]),
             weighted_batch, 550)
    add_case("maxcut_delta", dict(SMALL, delta=1.5), weighted_batch, 600)
    add_case("maxcut_int_ratio", dict(SMALL, ratio=3), undirected_batch, 650)
    add_case("maxcut_identity_acts", dict(SMALL, mp_act="identity", mlp_act="identity", act="identity"),
             weighted_batch, 700)
    add_case("maxcut_relu_layers", dict(SMALL, mp_act="relu", mlp_act="tanh"), loops_and_duplicates, 750)
    add_leftover_case("maxcut_leftovers", dict(SMALL, ratio=1, max_iter=2), 800)
    out = os.path.join(HERE, "golden_maxcut_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
