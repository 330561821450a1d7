#!/usr/bin/env python3
"""Generate the golden vectors of LaPool (``tests/golden/golden_lapool_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_kmis.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs ``LaPooling`` on small
seeded inputs.  The reference's selector needs one leaf the stand-in does not have, torch_scatter's ``scatter_mul``; it
is supplied here, written from the package's published behaviour, by assigning into the imported reference module.

The leader set is a float comparison, so a case is kept only if
  (a) every decision v_i against a neighbour's v_j is separated by at least 1e-5 relative (the project's fp32 tolerance:
      rounding on another device cannot flip such a case), and
  (b) a float64 run of the reference gives the same leader set.
Seeds are walked until a case passes both; the seed is stored.  Every case also stores a float64 run: v, S, the pooled x
and the gradient of ``sum(x_pool ** 2)`` with respect to ``x``.  (v is not an output of the reference: it is recomputed
by ``tests/lapool_restatement.py`` in the layout the case runs in, float64.)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lapool.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import make_golden as G  # noqa: E402  (installs the PyG stand-in and imports the reference)
import tgp.select.lapool_select as RL  # noqa: E402
from make_golden_dmon import directed_graphs  # noqa: E402
import lapool_restatement as R  # noqa: E402


def _scatter_mul(src, index, dim=0, out=None, dim_size=None):  # torch_scatter 2.1.2: products per index, ones elsewhere
    size = dim_size if dim_size is not None else (int(index.max()) + 1 if index.numel() else 0)
    return src.new_ones(size).scatter_reduce_(0, index, src, reduce="prod", include_self=True)


RL.scatter_mul = _scatter_mul

from tgp.poolers.lapool import LaPooling  # noqa: E402

CASES = {}


def run(cfg, inputs, double=False):
    kw = {k: (v.double() if double and isinstance(v, torch.Tensor) and v.is_floating_point() else v)
          for k, v in inputs.items()}
    x = kw.pop("x").clone().requires_grad_(True)
    if "edge_index" in kw:
        kw["adj"] = kw.pop("edge_index")
    pooler = LaPooling(**cfg).eval()
    return x, pooler(x=x, **kw)


def own_view(cfg, inputs, dtype):
    """(v, leader mask) from the restatement in the layout the case runs in."""
    x = inputs["x"].to(dtype)
    if inputs.get("adj") is not None:  # a dense call
        a, m = inputs["adj"].to(dtype), inputs.get("mask")
        v = R.variation(x, a, m)
        return v, R.leaders_from(v, a, m), a, m, x, None
    ei, ew, batch = inputs["edge_index"], inputs.get("edge_weight"), inputs.get("batch")
    ew = None if ew is None else ew.to(dtype)
    if not cfg.get("batched", True):
        v = R.variation(x, edge_index=ei, edge_weight=ew)
        return v, R.leaders_from(v, edge_index=ei, batch=batch), None, None, x, batch
    # batched over a sparse input: the reference densifies first (duplicates summed, explicit zeros no neighbours)
    b = batch if batch is not None else torch.zeros(x.size(0), dtype=torch.long)
    sizes = torch.bincount(b)
    ptr = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])
    B, N = sizes.numel(), int(sizes.max())
    a = torch.zeros(B, N, N, dtype=dtype)
    w = torch.ones(ei.size(1), dtype=dtype) if ew is None else ew.reshape(-1)
    a.index_put_((b[ei[0]], ei[0] - ptr[b[ei[0]]], ei[1] - ptr[b[ei[1]]]), w, accumulate=True)
    xd = torch.zeros(B, N, x.size(1), dtype=dtype)
    loc = torch.arange(x.size(0)) - ptr[b]
    xd[b, loc] = x
    m = torch.zeros(B, N, dtype=torch.bool)
    m[b, loc] = True
    v = R.variation(xd, a, m)
    return v, R.leaders_from(v, a, m), a, m, xd, None


def separated(v, a, m, inputs, cfg):
    """(a): every compared pair differs by at least 1e-5 relative."""
    if a is not None:
        nb = (a != 0) & m.unsqueeze(1) & m.unsqueeze(2)
        nb = nb & ~torch.eye(a.size(1), dtype=torch.bool).unsqueeze(0)
        vi, vj = v.unsqueeze(2).expand_as(nb)[nb], v.unsqueeze(1).expand_as(nb)[nb]
    else:
        ei = inputs["edge_index"]
        keep = ei[0] != ei[1]
        vi, vj = v[ei[0][keep]], v[ei[1][keep]]
    if vi.numel() == 0:
        return True
    gap = (vi - vj).abs() / torch.maximum(vi.abs(), vj.abs()).clamp_min(1e-30)
    return float(gap.min()) >= 1e-5


def add_case(name, cfg, make_inputs, first_seed):
    for seed in range(first_seed, first_seed + 200):
        inputs = make_inputs(seed)
        v32, lead32, a, m, xs32, sb = own_view(cfg, inputs, torch.float32)
        v64, lead64, _, _, xs64, _ = own_view(cfg, inputs, torch.float64)
        if separated(v32, a, m, inputs, cfg) and torch.equal(lead32, lead64):
            break
    else:
        raise RuntimeError(f"{name}: no seed gave a well-separated leader set")
    with torch.no_grad():
        _, out = run(cfg, inputs)
    x64, out64 = run(cfg, inputs, double=True)
    # the reference chose the same leaders, in float32 and in float64: its S is the restatement's for that leader set
    for got, xs, lead, tol in ((out.so.s, xs32, lead32, 1e-6), (out64.so.s, xs64, lead64, 1e-12)):
        want = R.assign(xs, lead, mask=m, batch=sb)
        assert got.shape == want.shape, f"{name}: S {tuple(got.shape)} against {tuple(want.shape)}"
        torch.testing.assert_close(got, want, rtol=tol, atol=tol)
    (g64,) = torch.autograd.grad((out64.x ** 2).sum(), x64)
    exp = G.pool_dict(out)
    exp["so"]["leader_mask"] = G.t(lead32)
    if cfg.get("s_inv_op") == "inverse":
        exp["so"]["s_inv"] = G.t(out.so.s_inv)
    CASES[name] = {"kind": "pool", "seed": seed, "inputs": {k: G.t(v) for k, v in inputs.items()}, "cfg": cfg,
                   "expected": exp,
                   "f64": {"v": G.t(v64), "s": G.t(out64.so.s), "x": G.t(out64.x), "grads": {"x": G.t(g64)}}}
    print(f"{name}: seed {seed}, x {tuple(inputs['x'].shape)}, S {tuple(out.so.s.shape)}, "
          f"leaders {int(lead32.sum())}")


# ---- inputs ----------------------------------------------------------------------------------------------------------
def graphs_batch(seed, p=0.15, top=40):
    gen = torch.Generator().manual_seed(seed)
    nb = int(torch.randint(4, 7, (1,), generator=gen))
    sizes = torch.randint(5, top + 1, (nb,), generator=gen).tolist()
    x, ei, ew, batch = G.batched_graphs(sizes, p, gen, 4, True)
    return dict(x=x, edge_index=ei, edge_weight=ew, batch=batch)


def single_graph(seed):
    gen = torch.Generator().manual_seed(seed)
    ei, ew = G.er_graph(30, 0.15, gen, True)
    return dict(x=torch.randn(30, 4, generator=gen), edge_index=ei, edge_weight=ew, batch=None)


def directed_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(5, 31, (4,), generator=gen).tolist()
    x, ei, ew, batch = directed_graphs(sizes, 0.12, gen, 4)
    return dict(x=x, edge_index=ei, edge_weight=ew, batch=batch)


def small_batch(seed):
    """4-6 graphs of 5-20 nodes: the cases that are about something other than size (the file stays small)."""
    return graphs_batch(seed, p=0.25, top=20)


def messy_batch(seed):
    """Self-loops, duplicate edges and one explicit zero weight; the list is grouped by graph, unordered inside one."""
    d = small_batch(seed)
    ei, ew = d["edge_index"], d["edge_weight"]
    gen = torch.Generator().manual_seed(seed + 7)
    n = d["x"].size(0)
    loops = torch.randperm(n, generator=gen)[: max(2, n // 6)]
    dup = torch.randperm(ei.size(1), generator=gen)[: max(2, ei.size(1) // 8)]
    d["edge_index"] = torch.cat([ei, torch.stack([loops, loops]), ei[:, dup]], 1).contiguous()
    ew = torch.cat([ew, torch.rand(loops.numel(), generator=gen) + 0.1, torch.rand(dup.numel(), generator=gen) + 0.1])
    ew[int(torch.randint(0, ei.size(1), (1,), generator=gen))] = 0.0
    # grouped by graph again (PyG's unbatch_edge_index splits the list by per-graph counts), unordered inside a graph
    order = torch.sort(d["batch"][d["edge_index"][0]], stable=True).indices
    d["edge_index"], d["edge_weight"] = d["edge_index"][:, order].contiguous(), ew[order].contiguous()
    return d


def edgeless_batch(seed):
    d = small_batch(seed)
    ei, ew, batch = d["edge_index"], d["edge_weight"], d["batch"]
    keep = (batch[ei[0]] != 1) & (ei[0] % 7 != 3) & (ei[1] % 7 != 3)  # graph 1 loses its edges, every 7th node its own
    d["edge_index"], d["edge_weight"] = ei[:, keep].contiguous(), ew[keep].contiguous()
    return d


def dense_masked(seed):
    """An already padded batch: sizes 12, 7, 1, 9 of N = 12, symmetric weights, junk in the padded rows and columns."""
    gen = torch.Generator().manual_seed(seed)
    sizes, N = [12, 7, 1, 9], 12
    up = torch.triu((torch.rand(4, N, N, generator=gen) < 0.3).float() * (torch.rand(4, N, N, generator=gen) + 0.1), 1)
    mask = torch.arange(N).unsqueeze(0) < torch.tensor(sizes).unsqueeze(1)
    return dict(x=torch.randn(4, N, 4, generator=gen), adj=up + up.transpose(1, 2), mask=mask)


def main():
    for batched in (True, False):
        for sparse_out in (False, True):
            tag = f"{'batched' if batched else 'unbatched'}_{'sparse' if sparse_out else 'dense'}out"
            base = dict(batched=batched, sparse_output=sparse_out)
            add_case(f"lapool_batch_{tag}", base, graphs_batch, 100)
            add_case(f"lapool_messy_{tag}", base, messy_batch, 300)
            add_case(f"lapool_edgeless_{tag}", base, edgeless_batch, 400)
        add_case(f"lapool_single_{'batched' if batched else 'unbatched'}", dict(batched=batched), single_graph, 200)
        add_case(f"lapool_directed_{'batched' if batched else 'unbatched'}", dict(batched=batched), directed_batch, 500)
    add_case("lapool_dense_mask", dict(batched=True), dense_masked, 600)
    add_case("lapool_dense_mask_sparseout", dict(batched=True, sparse_output=True), dense_masked, 600)
    add_case("lapool_keep_self_loops", dict(batched=True, remove_self_loops=False), messy_batch, 700)
    add_case("lapool_no_degree_norm", dict(batched=False, degree_norm=False), small_batch, 720)
    add_case("lapool_edge_weight_norm", dict(batched=True, edge_weight_norm=True), small_batch, 740)
    add_case("lapool_s_inv_inverse", dict(batched=True, s_inv_op="inverse"), small_batch, 760)
    out = os.path.join(HERE, "golden_lapool_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
