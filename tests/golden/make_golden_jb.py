#!/usr/bin/env python3
"""Generate the golden vectors of Just Balance pooling (``tests/golden/golden_jb_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_dmon.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs
``get_pooler("jb")`` / ``get_pooler("jb_u")`` and the two Just Balance loss functions on small seeded inputs.  Every
pooler case also stores a float64 run of the reference (pooler and inputs ``.double()``): its loss and the gradients of
that loss with respect to ``x`` and the selector parameters.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_jb.py
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
LOSS = "balance_loss"


def f64_run(alias, cfg, params, inputs):
    """The reference in float64: its loss and d loss / d x, d loss / d selector parameters."""
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
    v = out.loss[LOSS]
    g = torch.autograd.grad(v, leaves, allow_unused=True)
    grads = {"x": G.t(g[0] if g[0] is not None else torch.zeros_like(x)),
             "params": {n: G.t(gi if gi is not None else torch.zeros_like(p))
                        for n, gi, p in zip(names, g[1:], leaves[1:])}}
    return {"losses": {LOSS: v.detach().clone()}, "grads": {LOSS: grads}}


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


FLAG_SETS = (
    ("default", dict()),
    ("sparse_out", dict(sparse_output=True)),
    ("noT_ewn", dict(adj_transpose=False, edge_weight_norm=True)),
    ("raw", dict(remove_self_loops=False, degree_norm=False)),
    ("mlp2", dict(in_channels=[5, 7], act="relu")),
    ("nonorm", dict(normalize_loss=False)),
    ("coeff05", dict(loss_coeff=0.5)),
)


def gen_poolers():
    sizes = [9, 6, 12]
    for alias, mode, seed, pseed in (("jb", "batched", 3, 1), ("jb_u", "unbatched", 4, 2)):
        for tag, flags in FLAG_SETS:
            for weighted in (True, False):
                gen = torch.Generator().manual_seed(seed)
                x, ei, ew, batch = G.batched_graphs(sizes, 0.4, gen, 5, weighted)
                cfg = dict(in_channels=5, k=4)
                cfg.update(flags)
                add_pool(f"jb_{mode}_{tag}_{'w' if weighted else 'u'}", alias, cfg,
                         dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), pseed)
    # single graph, no batch vector, both modes
    gen = torch.Generator().manual_seed(6)
    ei, ew = G.er_graph(10, 0.4, gen, True)
    x = torch.randn(10, 5, generator=gen)
    for mode in ("", "_u"):
        add_pool(f"jb{mode}_single_graph", "jb" + mode, dict(in_channels=5, k=3),
                 dict(x=x, edge_index=ei, edge_weight=ew, batch=None), 3)
    # already-dense padded inputs + explicit mask; "dirty": the masked rows of x are not zero (the selector masks S)
    gen = torch.Generator().manual_seed(8)
    B, N, F = 3, 8, 5
    a = (torch.rand(B, N, N, generator=gen) < 0.4).float() * torch.rand(B, N, N, generator=gen)
    a = a + a.transpose(1, 2)
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[1, 6:] = False
    mask[2, 5:] = False
    x_dirty = torch.randn(B, N, F, generator=gen)
    xd = x_dirty * mask.unsqueeze(-1)
    clean = a * mask.unsqueeze(1) * mask.unsqueeze(2)
    add_pool("jb_dense_inputs_mask", "jb", dict(in_channels=F, k=3), dict(x=xd, adj=clean, mask=mask), 4)
    add_pool("jb_dense_inputs_mask_dirty_x", "jb", dict(in_channels=F, k=3), dict(x=x_dirty, adj=clean, mask=mask), 4)
    add_pool("jb_dense_inputs_nomask", "jb", dict(in_channels=F, k=3), dict(x=xd, adj=clean), 4)


def gen_functions():
    """Both public losses on their own, float32 and float64.  ``s`` has zero masked rows and a zero column, ``s_dirty``
    masked rows that are not zero (an S handed in from outside: the loss sums all N rows, the mask only counts)."""
    gen = torch.Generator().manual_seed(21)
    B, N, Kc = 3, 7, 4
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[0, 5:] = False
    mask[2, 4:] = False
    s_dirty = torch.softmax(torch.randn(B, N, Kc, generator=gen), -1)
    s_dirty[:, :, 2] = 0.0  # a column no node is assigned to
    s = s_dirty * mask.unsqueeze(-1)
    _, _, _, batch = G.batched_graphs([6, 9, 5], 0.4, gen, 2, True)
    sf = torch.softmax(torch.randn(batch.numel(), Kc, generator=gen), -1)
    sf[:, 1] = 0.0
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        s_, sd_, sf_ = s.to(dt), s_dirty.to(dt), sf.to(dt)
        exp = {
            "mask": RL.just_balance_loss(s_, mask),
            "nomask": RL.just_balance_loss(s_),
            "dirty_mask": RL.just_balance_loss(sd_, mask),
            "dirty_nomask": RL.just_balance_loss(sd_),
            "mask_nonorm": RL.just_balance_loss(s_, mask, normalize_loss=False),
            "mask_sum": RL.just_balance_loss(s_, mask, batch_reduction="sum"),
            "dirty_mask_sum": RL.just_balance_loss(sd_, mask, batch_reduction="sum"),
            "nomask_n5_k6": RL.just_balance_loss(s_, num_nodes=5, num_supernodes=6),
            "mask_n5_k6": RL.just_balance_loss(s_, mask, num_nodes=5, num_supernodes=6),
            "unbatched": RL.unbatched_just_balance_loss(sf_, batch),
            "unbatched_nobatch": RL.unbatched_just_balance_loss(sf_),
            "unbatched_nonorm": RL.unbatched_just_balance_loss(sf_, batch, normalize_loss=False),
            "unbatched_sum": RL.unbatched_just_balance_loss(sf_, batch, batch_reduction="sum"),
        }
        CASES[f"jb_functions_{tag}"] = {
            "kind": "functions", "inputs": {"s": s_, "s_dirty": sd_, "mask": mask, "batch": batch, "s_flat": sf_},
            "expected": {k: G.t(v) for k, v in exp.items()}}


def main():
    gen_poolers()
    gen_functions()
    out = os.path.join(HERE, "golden_jb_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
