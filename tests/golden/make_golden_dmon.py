#!/usr/bin/env python3
"""Generate the golden vectors of DMoN pooling (``tests/golden/golden_dmon_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden.py`` (whose helpers it imports): the real reference (tgp 1.0.1) over the PyG stand-in
runs ``get_pooler("dmon")`` / ``get_pooler("dmon_u")`` and the four DMoN loss functions on small seeded inputs.  Every
pooler case also stores a float64 run of the reference (pooler and inputs ``.double()``): its three losses and, for
each loss alone, its gradients with respect to ``x`` and the selector parameters.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dmon.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as G  # noqa: E402  (installs the PyG stand-in and imports the reference)
from tgp.poolers import get_pooler  # noqa: E402
from tgp.utils import losses as RL  # noqa: E402

CASES = {}
LOSSES = ("spectral_loss", "cluster_loss", "ortho_loss")


def directed_graphs(sizes, p, gen, feat):
    """Weighted directed graphs: each direction of each pair is an edge with probability p, independently."""
    eis, ews, xs, bs, off = [], [], [], [], 0
    for g, n in enumerate(sizes):
        a = torch.rand(n, n, generator=gen) < p
        a.fill_diagonal_(False)
        ei = a.nonzero().t().contiguous()
        eis.append(ei + off)
        ews.append(torch.rand(ei.size(1), generator=gen) + 0.1)
        xs.append(torch.randn(n, feat, generator=gen))
        bs.append(torch.full((n,), g, dtype=torch.long))
        off += n
    return torch.cat(xs), torch.cat(eis, 1), torch.cat(ews), torch.cat(bs)


def f64_run(alias, cfg, params, inputs):
    """The reference in float64: its losses and, per loss, d loss / d x and d loss / d selector parameters."""
    pooler = get_pooler(alias, **cfg).double().eval()
    pooler.load_state_dict({k: v.double() for k, v in params.items()})
    kw = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in inputs.items()}
    x = kw.pop("x").clone().requires_grad_(True)
    if "edge_index" in kw:
        kw["adj"] = kw.pop("edge_index")
        if kw.get("edge_weight") is None:  # (the stand-in densifies with float32 ones otherwise)
            kw["edge_weight"] = torch.ones(kw["adj"].size(1), dtype=torch.float64)
    out = pooler(x=x, **kw)
    names = [n for n, _ in pooler.named_parameters()]
    leaves = [x] + [p for _, p in pooler.named_parameters()]
    losses, grads = {}, {}
    for name in LOSSES:
        v = out.loss[name]
        losses[name] = v.detach().clone()
        g = torch.autograd.grad(v, leaves, retain_graph=True, allow_unused=True)
        grads[name] = {"x": G.t(g[0] if g[0] is not None else torch.zeros_like(x)),
                       "params": {n: G.t(gi if gi is not None else torch.zeros_like(p))
                                  for n, gi, p in zip(names, g[1:], leaves[1:])}}
    return {"losses": losses, "grads": grads}


def add_pool(name, alias, cfg, inputs, seed):
    torch.manual_seed(seed)
    pooler = get_pooler(alias, **cfg).eval()
    kw = dict(inputs)
    if "edge_index" in kw:
        kw["adj"] = kw.pop("edge_index")
    with torch.no_grad():
        out = pooler(**kw)
    params = G.params_of(pooler)
    assert name not in CASES, name
    CASES[name] = {"kind": "pool", "alias": alias, "inputs": {k: G.t(v) for k, v in inputs.items()},
                   "params": params, "cfg": cfg, "expected": G.pool_dict(out), "f64": f64_run(alias, cfg, params, inputs)}


def gen_poolers():
    sizes = [9, 6, 12]
    for tag, flags in (
        ("default", dict()),
        ("sparse_out", dict(sparse_output=True)),
        ("noT_ewn", dict(adj_transpose=False, edge_weight_norm=True)),
        ("raw", dict(remove_self_loops=False, degree_norm=False)),
        ("mlp2", dict(in_channels=[5, 7], act="relu")),
    ):
        for weighted in (True, False):
            gen = torch.Generator().manual_seed(3)
            x, ei, ew, batch = G.batched_graphs(sizes, 0.4, gen, 5, weighted)
            cfg = dict(in_channels=5, k=4)
            cfg.update(flags)
            add_pool(f"dmon_batched_{tag}_{'w' if weighted else 'u'}", "dmon", cfg,
                     dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 1)
    gen = torch.Generator().manual_seed(3)
    x, ei, ew, batch = G.batched_graphs(sizes, 0.4, gen, 5, True)
    add_pool("dmon_batched_ortho1_w", "dmon", dict(in_channels=5, k=4, ortho_loss_coeff=1.0),
             dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 1)
    for tag, flags in (("default", dict()), ("sparse_out", dict(sparse_output=True)),
                       ("sparse_out_ewn", dict(sparse_output=True, edge_weight_norm=True))):
        for weighted in (True, False):
            gen = torch.Generator().manual_seed(4)
            x, ei, ew, batch = G.batched_graphs(sizes, 0.4, gen, 5, weighted)
            cfg = dict(in_channels=5, k=4, ortho_loss_coeff=1.0)
            cfg.update(flags)
            add_pool(f"dmon_unbatched_{tag}_{'w' if weighted else 'u'}", "dmon_u", cfg,
                     dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 2)
    # single graph, no batch vector, both modes
    gen = torch.Generator().manual_seed(6)
    ei, ew = G.er_graph(10, 0.4, gen, True)
    x = torch.randn(10, 5, generator=gen)
    for mode in ("", "_u"):
        add_pool(f"dmon{mode}_single_graph", "dmon" + mode, dict(in_channels=5, k=3),
                 dict(x=x, edge_index=ei, edge_weight=ew, batch=None), 3)
    # already-dense padded inputs + explicit mask; "dirty": the padded rows of A are not zero (the degrees are masked)
    gen = torch.Generator().manual_seed(8)
    B, N, F = 3, 8, 5
    a = (torch.rand(B, N, N, generator=gen) < 0.4).float() * torch.rand(B, N, N, generator=gen)
    a = a + a.transpose(1, 2)
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[1, 6:] = False
    mask[2, 5:] = False
    xd = torch.randn(B, N, F, generator=gen) * mask.unsqueeze(-1)
    clean = a * mask.unsqueeze(1) * mask.unsqueeze(2)
    add_pool("dmon_dense_inputs_mask", "dmon", dict(in_channels=F, k=3), dict(x=xd, adj=clean, mask=mask), 4)
    add_pool("dmon_dense_inputs_mask_dirty", "dmon", dict(in_channels=F, k=3), dict(x=xd, adj=a, mask=mask), 4)
    add_pool("dmon_dense_inputs_nomask", "dmon", dict(in_channels=F, k=3), dict(x=xd, adj=clean), 4)
    # directed weighted batch: the batched (in-degree) and unbatched (out-degree) modes disagree
    gen = torch.Generator().manual_seed(11)
    x, ei, ew, batch = directed_graphs(sizes, 0.4, gen, 5)
    for mode in ("", "_u"):
        add_pool(f"dmon{mode}_directed_w", "dmon" + mode, dict(in_channels=5, k=4),
                 dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 1)
    # a batch with an edgeless graph (m = 0)
    gen = torch.Generator().manual_seed(12)
    x, ei, ew, batch = G.batched_graphs(sizes, 0.4, gen, 5, True)
    keep = batch[ei[0]] != 1
    ei, ew = ei[:, keep].contiguous(), ew[keep].contiguous()
    for mode in ("", "_u"):
        add_pool(f"dmon{mode}_edgeless_graph_w", "dmon" + mode, dict(in_channels=5, k=4),
                 dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 1)


def gen_functions():
    """Each public loss on its own, float32 and float64."""
    gen = torch.Generator().manual_seed(21)
    B, N, Kc = 3, 7, 4
    a = (torch.rand(B, N, N, generator=gen) < 0.5).float() * (torch.rand(B, N, N, generator=gen) + 0.1)
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[0, 5:] = False
    mask[2, 4:] = False
    s = torch.softmax(torch.randn(B, N, Kc, generator=gen), -1) * mask.unsqueeze(-1)
    x, ei, ew, batch = G.batched_graphs([6, 9, 5], 0.4, gen, 2, True)
    sf = torch.softmax(torch.randn(x.size(0), Kc, generator=gen), -1)
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        a_, s_, sf_, ew_ = a.to(dt), s.to(dt), sf.to(dt), ew.to(dt)
        raw = s_.transpose(1, 2) @ a_ @ s_
        exp = {
            "spectral_mask": RL.spectral_loss(a_, s_, raw, mask),
            "spectral_nomask": RL.spectral_loss(a_, s_, raw),
            "cluster_mask": RL.cluster_loss(s_, mask=mask),
            "cluster_nomask": RL.cluster_loss(s_),
            "cluster_sum": RL.cluster_loss(s_, mask=mask, batch_reduction="sum"),
            "sparse_spectral_w": RL.sparse_spectral_loss(ei, sf_, ew_, batch),
            "sparse_spectral_u": RL.sparse_spectral_loss(ei, sf_, None, batch),
            "sparse_spectral_nobatch": RL.sparse_spectral_loss(ei[:, batch[ei[0]] == 0], sf_[:6], ew_[batch[ei[0]] == 0]),
            "unbatched_cluster": RL.unbatched_cluster_loss(sf_, batch),
            "unbatched_cluster_nobatch": RL.unbatched_cluster_loss(sf_),
        }
        CASES[f"dmon_functions_{tag}"] = {
            "kind": "functions", "inputs": {"adj": a_, "s": s_, "raw": raw, "mask": mask, "edge_index": ei,
                                            "edge_weight": ew_, "batch": batch, "s_flat": sf_},
            "expected": {k: G.t(v) for k, v in exp.items()}}


def main():
    gen_poolers()
    gen_functions()
    out = os.path.join(HERE, "golden_dmon_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
