#!/usr/bin/env python3
"""Generate the golden vectors of HOSC pooling (``tests/golden/golden_hosc_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_dmon.py`` (whose helpers it imports): the real reference (tgp 1.0.1) over the PyG stand-in
runs ``get_pooler("hosc")`` / ``get_pooler("hosc_u")`` and the three HOSC loss functions on small seeded inputs.  Every
pooler case also stores a float64 run of the reference (pooler and inputs ``.double()``): its two losses and, for each
loss alone, its gradients with respect to ``x`` and the selector parameters.

Where the reference hands out an int64 zero for a disabled term (``mu = 0``), the fixture stores that zero in the run's
floating dtype; a loss that does not depend on the leaves has zero gradients.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hosc.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as G  # noqa: E402  (installs the PyG stand-in and imports the reference)
from make_golden_dmon import directed_graphs  # noqa: E402
from tgp.poolers import get_pooler  # noqa: E402
from tgp.utils import losses as RL  # noqa: E402

CASES = {}
LOSSES = ("hosc_loss", "ortho_loss")


def _as_float(v, dtype):
    v = v if isinstance(v, torch.Tensor) else torch.tensor(v)
    return v.detach().to(dtype).clone()


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
        losses[name] = _as_float(v, torch.float64)
        if isinstance(v, torch.Tensor) and v.requires_grad:
            g = torch.autograd.grad(v, leaves, retain_graph=True, allow_unused=True)
        else:
            g = [None] * len(leaves)
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
    expected = G.pool_dict(out)
    expected["loss"] = {k: _as_float(v, torch.float32) for k, v in out.loss.items()}
    assert name not in CASES, name
    CASES[name] = {"kind": "pool", "alias": alias, "inputs": {k: G.t(v) for k, v in inputs.items()},
                   "params": params, "cfg": cfg, "expected": expected, "f64": f64_run(alias, cfg, params, inputs)}


def gen_poolers():
    sizes = [9, 6, 12]
    gen = torch.Generator().manual_seed(11)
    x, ei, ew, batch = directed_graphs(sizes, 0.4, gen, 5)
    for mode in ("", "_u"):
        for tag, flags in (
            ("default", dict()),
            ("hosc_ortho", dict(hosc_ortho=True)),
            ("alpha1", dict(alpha=1.0)),
            ("alpha0_mu0", dict(alpha=0.0, mu=0.0)),
            ("k1_hosc_ortho", dict(k=1, hosc_ortho=True)),
            ("sparse_out", dict(sparse_output=True)),
            ("noT_ewn", dict(adj_transpose=False, edge_weight_norm=True)),
            ("raw", dict(remove_self_loops=False, degree_norm=False)),
            ("mlp2", dict(in_channels=[5, 7], act="relu")),
        ):
            cfg = dict(in_channels=5, k=4)
            cfg.update(flags)
            add_pool(f"hosc{mode}_{tag}", "hosc" + mode, cfg, dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 1)
        add_pool(f"hosc{mode}_unweighted", "hosc" + mode, dict(in_channels=5, k=4),
                 dict(x=x, edge_index=ei, edge_weight=None, batch=batch), 1)
    # single graph, no batch vector, both modes
    gen = torch.Generator().manual_seed(6)
    xs, eis, ews, _ = directed_graphs([10], 0.4, gen, 5)
    for mode in ("", "_u"):
        add_pool(f"hosc{mode}_single_graph", "hosc" + mode, dict(in_channels=5, k=3),
                 dict(x=xs, edge_index=eis, edge_weight=ews, batch=None), 3)
    # a batch with an edgeless graph
    keep = batch[ei[0]] != 1
    ei2, ew2 = ei[:, keep].contiguous(), ew[keep].contiguous()
    for mode in ("", "_u"):
        for tag, flags in (("", dict()), ("_hosc_ortho", dict(hosc_ortho=True))):
            add_pool(f"hosc{mode}_edgeless_graph{tag}", "hosc" + mode, dict(in_channels=5, k=4, **flags),
                     dict(x=x, edge_index=ei2, edge_weight=ew2, batch=batch), 1)
    # already-dense padded inputs + explicit mask; "dirty": the padded rows and columns of A are not zero
    gen = torch.Generator().manual_seed(8)
    B, N, F = 3, 8, 5
    a = (torch.rand(B, N, N, generator=gen) < 0.4).float() * torch.rand(B, N, N, generator=gen)
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[1, 6:] = False
    mask[2, 5:] = False
    xd = torch.randn(B, N, F, generator=gen) * mask.unsqueeze(-1)
    clean = a * mask.unsqueeze(1) * mask.unsqueeze(2)
    for tag, flags in (("", dict()), ("_hosc_ortho", dict(hosc_ortho=True))):
        add_pool(f"hosc_dense_inputs_mask{tag}", "hosc", dict(in_channels=F, k=3, **flags),
                 dict(x=xd, adj=clean, mask=mask), 4)
        add_pool(f"hosc_dense_inputs_mask_dirty{tag}", "hosc", dict(in_channels=F, k=3, **flags),
                 dict(x=xd, adj=a, mask=mask), 4)
    add_pool("hosc_dense_inputs_nomask", "hosc", dict(in_channels=F, k=3, hosc_ortho=True), dict(x=xd, adj=clean), 4)


def gen_functions():
    """Each public loss on its own, float32 and float64."""
    gen = torch.Generator().manual_seed(21)
    B, N, Kc = 3, 7, 4
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[0, 5:] = False
    mask[2, 4:] = False
    s = torch.softmax(torch.randn(B, N, Kc, generator=gen), -1) * mask.unsqueeze(-1)
    x, ei, ew, batch = directed_graphs([6, 9, 5], 0.4, gen, 2)
    sf = torch.softmax(torch.randn(x.size(0), Kc, generator=gen), -1)
    one = batch[ei[0]] == 0
    none = ei[:, :0]
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        s_, sf_, ew_ = s.to(dt), sf.to(dt), ew.to(dt)
        exp = {
            "ortho_mask": RL.hosc_orthogonality_loss(s_, mask),
            "ortho_nomask": RL.hosc_orthogonality_loss(s_),
            "ortho_sum": RL.hosc_orthogonality_loss(s_, mask, batch_reduction="sum"),
            "ortho_k1": RL.hosc_orthogonality_loss(s_[:, :, :1], mask),
            "unbatched_ortho": RL.unbatched_hosc_orthogonality_loss(sf_, batch),
            "unbatched_ortho_sum": RL.unbatched_hosc_orthogonality_loss(sf_, batch, batch_reduction="sum"),
            "unbatched_ortho_nobatch": RL.unbatched_hosc_orthogonality_loss(sf_),
            "unbatched_ortho_k1": RL.unbatched_hosc_orthogonality_loss(sf_[:, :1], batch),
            "ho_w": RL.sparse_ho_mincut_loss(ei, sf_, ew_, batch),
            "ho_u": RL.sparse_ho_mincut_loss(ei, sf_, None, batch),
            "ho_sum": RL.sparse_ho_mincut_loss(ei, sf_, ew_, batch, batch_reduction="sum"),
            "ho_nobatch": RL.sparse_ho_mincut_loss(ei[:, one], sf_[:6], ew_[one]),
            "ho_nobatch_sum": RL.sparse_ho_mincut_loss(ei[:, one], sf_[:6], ew_[one], batch_reduction="sum"),
            "ho_no_edges": RL.sparse_ho_mincut_loss(none, sf_, None, batch),
            "ho_no_edges_nobatch": RL.sparse_ho_mincut_loss(none, sf_[:6], None),
        }
        CASES[f"hosc_functions_{tag}"] = {
            "kind": "functions", "inputs": {"s": s_, "mask": mask, "edge_index": ei, "edge_weight": ew_, "batch": batch,
                                            "s_flat": sf_},
            "expected": {k: G.t(v) for k, v in exp.items()}}


def main():
    gen_poolers()
    gen_functions()
    out = os.path.join(HERE, "golden_hosc_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
