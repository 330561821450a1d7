#!/usr/bin/env python3
"""Generate the golden vectors of GTVConv (``tests/golden/golden_gtv_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_pan.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs its own
``GTVConv.forward`` on small seeded inputs.  The stand-in has neither ``MessagePassing`` nor ``nn.inits.zeros``; a
minimal form of both is registered HERE (the stand-in's file is not edited) before ``tgp.mp.gtvconv`` is imported: a
``torch.nn.Module`` whose ``propagate(edge_index, x, edge_weight, size)`` is
``zeros.index_add_(0, edge_index[0], self.message(x[edge_index[1]], edge_weight))`` -- the layer's own
``flow="target_to_source"`` with ``aggr="add"``.  Nothing of the forward was replaced.  (One case is fed differently:
see ``connectivity`` on the torch COO adjacency.)

Every case stores the inputs and parameters, the float32 output, and a float64 run: the output, a fixed random upstream
gradient and the gradients it sends to ``x``, ``weight``, ``bias`` and ``edge_weight`` (dense cases: ``adj``).

Separation rule.  Seeds are walked until, for the projected ``h = x @ weight`` (float64), no non-loop edge has a channel
with ``0 < |h_ic - h_jc| < 1e-4`` and none has ``|d_e - eps| < 1e-4 eps``: the kinks of ``sign`` and ``clamp`` stay
away from float32 noise.  The seed is stored.

Per case the float32 reference's own normwise error against its float64 run is printed and stored (``e_ref32``); a case is
refused if 16 x that error exceeds the ``CAP`` of ``tests/test_gpu_grad_paths.py``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gtv.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import make_golden as G  # noqa: E402  (installs the PyG stand-in and imports the reference)


class MessagePassing(torch.nn.Module):
    """What GTVConv uses of PyG's class: ``aggr="add"``, ``flow="target_to_source"``, no explicit size."""

    def __init__(self, aggr="add", flow="source_to_target", **kwargs):
        super().__init__()
        assert aggr == "add" and flow == "target_to_source"

    def propagate(self, edge_index, x, edge_weight, size=None):
        assert size is None
        return torch.zeros_like(x).index_add_(0, edge_index[0], self.message(x[edge_index[1]], edge_weight))


def _zeros(value):
    if isinstance(value, torch.Tensor):
        value.data.fill_(0.0)


sys.modules["torch_geometric.nn"].MessagePassing = MessagePassing
sys.modules["torch_geometric.nn.inits"].zeros = _zeros

from tgp.mp.gtvconv import GTVConv  # noqa: E402
from tgp.utils.ops import connectivity_to_edge_index  # noqa: E402
from make_golden_dmon import directed_graphs  # noqa: E402

import gtv_restatement as R  # noqa: E402
from test_gpu_grad_paths import CAP, FACTOR  # noqa: E402

CASES = {}
F_IN, F_OUT = 5, 6


def connectivity(inputs, dtype, grad=False):
    """(the layer's second argument, its edge_weight argument, the leaf that carries the edge values or None)."""
    if "adj" in inputs:
        adj = inputs["adj"].to(dtype)
        if grad:
            adj = adj.clone().requires_grad_(True)
        return adj, None, adj
    w = inputs.get("edge_weight")
    if w is not None:
        w = w.to(dtype)
        if grad:
            w = w.clone().requires_grad_(True)
    if inputs.get("coo"):
        # The reference's forward reads every tensor whose last two sizes agree as a dense adjacency, so a square torch
        # COO tensor never reaches its sparse branch (torch.nonzero has no sparse form).  The case therefore runs what
        # that branch does first -- the reference's own connectivity_to_edge_index on the COO tensor -- and hands the
        # result to the forward.
        n = inputs["x"].size(0)
        ei, values = connectivity_to_edge_index(torch.sparse_coo_tensor(inputs["edge_index"], w, (n, n)).coalesce())
        return ei, values, w
    return inputs["edge_index"], w, w


def run(cfg, params, inputs, dtype, grad=False):
    conv = GTVConv(**cfg).to(dtype)
    with torch.no_grad():
        conv.weight.copy_(params["weight"].to(dtype))
        if conv.bias is not None:
            conv.bias.copy_(params["bias"].to(dtype))
    x = inputs["x"].to(dtype)
    if grad:
        x = x.clone().requires_grad_(True)
    conn, ew, edge_leaf = connectivity(inputs, dtype, grad)
    out = conv(x, conn, ew, mask=inputs.get("mask"))
    return out, conv, x, edge_leaf


def separated(cfg, params, inputs):
    h = inputs["x"].double() @ params["weight"].double()
    if "adj" in inputs:
        adj = inputs["adj"] if inputs["adj"].dim() == 3 else inputs["adj"].unsqueeze(0)
        ei, _ = R.dense_edges(adj)
        h = h.reshape(-1, h.size(-1))
    else:
        ei = inputs["edge_index"]
    diff, d = R.distances(h, ei)
    eps = cfg.get("eps", 1e-3)
    return not bool(((diff > 0) & (diff < 1e-4)).any()) and not bool(((d - eps).abs() < 1e-4 * eps).any())


def add_case(name, cfg, make_inputs, first_seed):
    cfg = dict(in_channels=F_IN, out_channels=F_OUT, **cfg)
    for seed in range(first_seed, first_seed + 200):
        inputs = make_inputs(seed)
        gen = torch.Generator().manual_seed(seed + 1)
        params = {"weight": torch.randn(F_IN, F_OUT, generator=gen) * (2.0 / F_IN) ** 0.5}
        if cfg.get("bias", True):
            params["bias"] = torch.randn(F_OUT, generator=gen) * 0.3
        if separated(cfg, params, inputs):
            break
    else:
        raise RuntimeError(f"{name}: no seed kept the kinks away")
    with torch.no_grad():
        out32, _, _, _ = run(cfg, params, inputs, torch.float32)
    out64, conv, x, edge_leaf = run(cfg, params, inputs, torch.float64, grad=True)
    up = torch.randn(out64.shape, generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64)
    leaves = {"x": x, "weight": conv.weight}
    if conv.bias is not None:
        leaves["bias"] = conv.bias
    if edge_leaf is not None:
        leaves["adj" if "adj" in inputs else "edge_weight"] = edge_leaf
    grads = torch.autograd.grad(out64, list(leaves.values()), up, allow_unused=True)
    grads = {k: G.t(g if g is not None else torch.zeros_like(v)) for (k, v), g in zip(leaves.items(), grads)}
    e_ref32 = float(torch.linalg.vector_norm(out32.double() - out64)) / max(float(torch.linalg.vector_norm(out64)), 1e-300)
    if FACTOR * e_ref32 > CAP:
        raise RuntimeError(f"{name}: 16 x the float32 reference's error {e_ref32:.3e} exceeds the cap {CAP:g}")
    assert name not in CASES, name
    CASES[name] = {"seed": seed, "cfg": cfg, "inputs": {k: G.t(v) for k, v in inputs.items()},
                   "params": {k: G.t(v) for k, v in params.items()}, "expected": G.t(out32), "e_ref32": e_ref32,
                   "f64": {"out": G.t(out64), "upstream": up, "grads": grads}}
    ne = inputs["edge_index"].size(1) if "edge_index" in inputs else int((inputs["adj"] != 0).sum())
    print(f"{name}: seed {seed}, x {tuple(inputs['x'].shape)}, E={ne}, e_ref32 {e_ref32:.2e}")


# ------------------------------------------------------------------------------------------------------------ inputs
def undirected_batch(weighted, scale=1.0):
    def make(seed):
        gen = torch.Generator().manual_seed(seed)
        sizes = torch.randint(6, 15, (4,), generator=gen).tolist()
        x, ei, ew, _ = G.batched_graphs(sizes, 0.3, gen, F_IN, weighted)
        return dict(x=x * scale, edge_index=ei, edge_weight=ew)
    return make


def directed_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(6, 15, (4,), generator=gen).tolist()
    x, ei, ew, _ = directed_graphs(sizes, 0.2, gen, F_IN)
    return dict(x=x, edge_index=ei, edge_weight=ew)


def loops_duplicates_unsorted(seed):
    """The weighted undirected batch with a self-loop on every third node and every fifth edge listed twice, shuffled."""
    d = undirected_batch(True)(seed)
    gen = torch.Generator().manual_seed(seed + 7)
    loops = torch.arange(0, d["x"].size(0), 3)
    ei = torch.cat([d["edge_index"], torch.stack([loops, loops]), d["edge_index"][:, ::5]], 1)
    ew = torch.cat([d["edge_weight"], torch.rand(loops.numel(), generator=gen) + 0.1, d["edge_weight"][::5] * 0.5])
    order = torch.randperm(ei.size(1), generator=gen)
    return dict(x=d["x"], edge_index=ei[:, order].contiguous(), edge_weight=ew[order].contiguous())


def isolated_nodes(seed):
    """Nodes 2 and 5 and the last node of the batch have no edge at all."""
    d = undirected_batch(True)(seed)
    ei, n = d["edge_index"], d["x"].size(0)
    keep = torch.ones(ei.size(1), dtype=torch.bool)
    for v in (2, 5, n - 1):
        keep &= (ei[0] != v) & (ei[1] != v)
    return dict(x=d["x"], edge_index=ei[:, keep].contiguous(), edge_weight=d["edge_weight"][keep].contiguous())


def zero_distance(seed):
    """Nodes 0 and 1 carry the same features and are joined in both directions: d_e = 0 exactly."""
    d = undirected_batch(True)(seed)
    d["x"][1] = d["x"][0]
    gen = torch.Generator().manual_seed(seed + 9)
    d["edge_index"] = torch.cat([torch.tensor([[0, 1], [1, 0]]), d["edge_index"]], 1)
    d["edge_weight"] = torch.cat([torch.rand(2, generator=gen) + 0.1, d["edge_weight"]])
    return d


def one_node(seed):
    gen = torch.Generator().manual_seed(seed)
    return dict(x=torch.randn(1, F_IN, generator=gen), edge_index=torch.zeros(2, 0, dtype=torch.long), edge_weight=None)


def edgeless(seed):
    gen = torch.Generator().manual_seed(seed)
    return dict(x=torch.randn(7, F_IN, generator=gen), edge_index=torch.zeros(2, 0, dtype=torch.long), edge_weight=None)


def coo_adjacency(seed):
    """A directed weighted graph handed over as a torch COO adjacency (coalesced: row-major, no duplicates)."""
    d = directed_batch(seed)
    return dict(x=d["x"], edge_index=d["edge_index"], edge_weight=d["edge_weight"], coo=True)


def dense_batch(seed):
    """B = 3, N = 9: weighted directed entries, a self-loop on most diagonals, padded rows masked out.  The reference
    cancels a_ii / eps between the degree and the entry in float32, so its own error grows with the loop weights: they
    stay below 0.25, which keeps 16 x that error well inside the cap."""
    gen = torch.Generator().manual_seed(seed)
    B, n = 3, 9
    adj = (torch.rand(B, n, n, generator=gen) + 0.1) * (torch.rand(B, n, n, generator=gen) < 0.35)
    adj = adj + torch.diag_embed((torch.rand(B, n, generator=gen) * 0.2 + 0.05) * (torch.rand(B, n, generator=gen) < 0.7))
    mask = torch.ones(B, n, dtype=torch.bool)
    mask[1, 7:] = False
    mask[2, 5:] = False
    return dict(x=torch.randn(B, n, F_IN, generator=gen), adj=adj.contiguous(), mask=mask)


def dense_2d(seed):
    gen = torch.Generator().manual_seed(seed)
    n = 11
    upper = torch.triu(torch.rand(n, n, generator=gen) < 0.3, 1)
    adj = (upper | upper.t()).float()
    return dict(x=torch.randn(n, F_IN, generator=gen), adj=adj.contiguous())


def main():
    add_case("gtv_undirected_weighted", dict(act="relu"), undirected_batch(True), 100)
    add_case("gtv_undirected_unweighted", dict(act="relu"), undirected_batch(False), 150)
    add_case("gtv_directed_elu_delta", dict(act="elu", delta_coeff=0.311), directed_batch, 200)
    add_case("gtv_loops_duplicates_unsorted", dict(act="identity"), loops_duplicates_unsorted, 250)
    add_case("gtv_isolated_nodes_tanh", dict(act="tanh"), isolated_nodes, 300)
    add_case("gtv_zero_distance", dict(act="elu"), zero_distance, 350)
    add_case("gtv_one_node", dict(act="relu"), one_node, 400)
    add_case("gtv_edgeless", dict(act="tanh", delta_coeff=0.311), edgeless, 450)
    add_case("gtv_no_bias", dict(act="relu", bias=False), undirected_batch(True), 500)
    add_case("gtv_eps_half", dict(act="identity", eps=0.5), undirected_batch(True, scale=0.05), 550)
    add_case("gtv_coo_adjacency", dict(act="relu", delta_coeff=0.311), coo_adjacency, 600)
    add_case("gtv_dense_batch_mask", dict(act="relu"), dense_batch, 650)
    add_case("gtv_dense_2d", dict(act="elu", delta_coeff=0.311, bias=False), dense_2d, 700)
    out = os.path.join(HERE, "golden_gtv_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
