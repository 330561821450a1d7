#!/usr/bin/env python3
"""Generate the golden vectors of AsymCheegerCut pooling (``tests/golden/golden_acc_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_dmon.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs ``get_pooler("acc")``
/ ``get_pooler("acc_u")`` and the four ACC loss functions on small seeded inputs.  Every pooler case also stores a
float64 run of the reference (pooler and inputs ``.double()``): its two losses and, for each loss alone, its gradients
with respect to ``x`` and the selector parameters.

The inputs are standard-normal and the selectors keep their default initialisation, so no column of S has two nodes
tied at its quantile; ``assert_no_quantile_tie`` checks that for every case, so that the tie rule (the reference's
unstable sort leaves it open) never decides a stored value.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_acc.py
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
LOSSES = ("total_variation_loss", "balance_loss")


def assert_no_quantile_tie(s, k, graph, name):
    """``s`` [rows,K] with the graph id of every row: in no graph does a column hold its quantile value twice."""
    if k <= 1:
        return
    for g in graph.unique().tolist():
        rows = s[graph == g]
        n = rows.size(0)
        if n == 0:
            continue
        q = rows.sort(dim=0, descending=True)[0][min(n // k, n - 1)]
        assert int((rows == q).sum(0).max()) == 1, f"{name}: graph {g} has a tie at a column's quantile"


def check_ties(name, out, k, inputs):
    s = out.so.s.detach()
    if s.dim() == 3:
        mask = out.so.in_mask if getattr(out.so, "in_mask", None) is not None else inputs.get("mask")
        if mask is None:
            mask = torch.ones(s.shape[:2], dtype=torch.bool)
        graph = torch.arange(s.size(0)).unsqueeze(1).expand(s.shape[:2])[mask]
        assert_no_quantile_tie(s[mask], k, graph, name)
    else:
        batch = inputs.get("batch")
        graph = batch if batch is not None else torch.zeros(s.size(0), dtype=torch.long)
        assert_no_quantile_tie(s, k, graph, name)


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
        if v.requires_grad:
            g = torch.autograd.grad(v, leaves, retain_graph=True, allow_unused=True)
        else:  # (k = 1: the balance loss is a constant 0)
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
    check_ties(name, out, cfg["k"], inputs)
    params = G.params_of(pooler)
    assert name not in CASES, name
    CASES[name] = {"kind": "pool", "alias": alias, "inputs": {k: G.t(v) for k, v in inputs.items()},
                   "params": params, "cfg": cfg, "expected": G.pool_dict(out), "f64": f64_run(alias, cfg, params, inputs)}


def gen_poolers():
    sizes = [9, 6, 12]
    # undirected batches of variable size (the batched mode pads them and masks the padding)
    for tag, flags in (
        ("default", dict()),
        ("sparse_out", dict(sparse_output=True)),
        ("noT_ewn", dict(adj_transpose=False, edge_weight_norm=True)),
        ("coeffs", dict(totvar_coeff=0.5, balance_coeff=2.0)),
        ("mlp2", dict(in_channels=[5, 7], act="relu")),
    ):
        for weighted in (True, False):
            gen = torch.Generator().manual_seed(3)
            x, ei, ew, batch = G.batched_graphs(sizes, 0.4, gen, 5, weighted)
            cfg = dict(in_channels=5, k=4)
            cfg.update(flags)
            add_pool(f"acc_batched_{tag}_{'w' if weighted else 'u'}", "acc", cfg,
                     dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 1)
    for tag, flags in (("default", dict()), ("sparse_out", dict(sparse_output=True))):
        for weighted in (True, False):
            gen = torch.Generator().manual_seed(4)
            x, ei, ew, batch = G.batched_graphs(sizes, 0.4, gen, 5, weighted)
            cfg = dict(in_channels=5, k=4)
            cfg.update(flags)
            add_pool(f"acc_unbatched_{tag}_{'w' if weighted else 'u'}", "acc_u", cfg,
                     dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 2)
    # single graph, no batch vector, both modes
    gen = torch.Generator().manual_seed(6)
    ei, ew = G.er_graph(10, 0.4, gen, True)
    x = torch.randn(10, 5, generator=gen)
    for mode in ("", "_u"):
        add_pool(f"acc{mode}_single_graph", "acc" + mode, dict(in_channels=5, k=3),
                 dict(x=x, edge_index=ei, edge_weight=ew, batch=None), 3)
    # already-dense padded inputs, with and without a mask
    gen = torch.Generator().manual_seed(8)
    B, N, F = 3, 8, 5
    a = (torch.rand(B, N, N, generator=gen) < 0.4).float() * torch.rand(B, N, N, generator=gen)
    a = a + a.transpose(1, 2)
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[1, 6:] = False
    mask[2, 5:] = False
    xd = torch.randn(B, N, F, generator=gen)
    clean = a * mask.unsqueeze(1) * mask.unsqueeze(2)
    add_pool("acc_dense_inputs_mask", "acc", dict(in_channels=F, k=3),
             dict(x=xd * mask.unsqueeze(-1), adj=clean, mask=mask), 4)
    add_pool("acc_dense_inputs_nomask", "acc", dict(in_channels=F, k=3), dict(x=xd, adj=a), 4)
    # weighted directed batch
    gen = torch.Generator().manual_seed(11)
    x, ei, ew, batch = directed_graphs(sizes, 0.4, gen, 5)
    for mode in ("", "_u"):
        add_pool(f"acc{mode}_directed_w", "acc" + mode, dict(in_channels=5, k=4),
                 dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 1)
    add_pool("acc_directed_noT_w", "acc", dict(in_channels=5, k=4, adj_transpose=False),
             dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 1)
    # a batch with an edgeless graph (E = 0, clamped to 1)
    gen = torch.Generator().manual_seed(12)
    x, ei, ew, batch = G.batched_graphs(sizes, 0.4, gen, 5, True)
    keep = batch[ei[0]] != 1
    ei2, ew2 = ei[:, keep].contiguous(), ew[keep].contiguous()
    for mode in ("", "_u"):
        add_pool(f"acc{mode}_edgeless_graph_w", "acc" + mode, dict(in_channels=5, k=4),
                 dict(x=x, edge_index=ei2, edge_weight=ew2, batch=batch), 1)
    # zero-weight edges: the edge form counts them, the dense form (nonzero entries) does not
    ew0 = ew.clone()
    ew0[::3] = 0.0
    for mode in ("", "_u"):
        add_pool(f"acc{mode}_zero_weight_edges", "acc" + mode, dict(in_channels=5, k=4),
                 dict(x=x, edge_index=ei, edge_weight=ew0, batch=batch), 1)
    # k = 1 (no balance term) and a graph with fewer nodes than clusters (idx = 0: the column maximum)
    for mode in ("", "_u"):
        add_pool(f"acc{mode}_k1", "acc" + mode, dict(in_channels=5, k=1),
                 dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 1)
    gen = torch.Generator().manual_seed(13)
    x, ei, ew, batch = G.batched_graphs([9, 3, 12], 0.5, gen, 5, True)
    for mode in ("", "_u"):
        add_pool(f"acc{mode}_n_lt_k", "acc" + mode, dict(in_channels=5, k=5),
                 dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 1)


def gen_functions():
    """Each public loss on its own, float32 and float64."""
    gen = torch.Generator().manual_seed(21)
    B, N, Kc = 3, 7, 4
    a = (torch.rand(B, N, N, generator=gen) < 0.5).float() * (torch.rand(B, N, N, generator=gen) + 0.1)
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[0, 5:] = False
    mask[2, 4:] = False
    a = a * mask.unsqueeze(1) * mask.unsqueeze(2)
    s = torch.softmax(torch.randn(B, N, Kc, generator=gen), -1) * mask.unsqueeze(-1)
    x, ei, ew, batch = G.batched_graphs([6, 9, 5], 0.4, gen, 2, True)
    ew[1::4] = 0.0
    sf = torch.softmax(torch.randn(x.size(0), Kc, generator=gen), -1)
    one = batch[ei[0]] == 0
    graph = torch.arange(B).unsqueeze(1).expand(B, N)
    assert_no_quantile_tie(s[mask], Kc, graph[mask], "functions.mask")
    assert_no_quantile_tie(sf, Kc, batch, "functions.flat")
    assert_no_quantile_tie(sf, Kc, torch.zeros_like(batch), "functions.flat_nobatch")
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        a_, s_, sf_, ew_ = a.to(dt), s.to(dt), sf.to(dt), ew.to(dt)
        exp = {
            "totvar": RL.totvar_loss(s_, a_),
            "totvar_sum": RL.totvar_loss(s_, a_, batch_reduction="sum"),
            "sparse_totvar_w": RL.sparse_totvar_loss(ei, sf_, ew_, batch),
            "sparse_totvar_u": RL.sparse_totvar_loss(ei, sf_, None, batch),
            "sparse_totvar_nobatch": RL.sparse_totvar_loss(ei[:, one], sf_[:6], ew_[one]),
            "asym_mask": RL.asym_norm_loss(s_, Kc, mask=mask),
            "asym_sum": RL.asym_norm_loss(s_, Kc, mask=mask, batch_reduction="sum"),
            "asym_k1": RL.asym_norm_loss(s_, 1),
            "asym_k9": RL.asym_norm_loss(s_[:, :5], 9, mask=mask[:, :5]),
            "unbatched_asym": RL.unbatched_asym_norm_loss(sf_, Kc, batch),
            "unbatched_asym_nobatch": RL.unbatched_asym_norm_loss(sf_, Kc),
            "unbatched_asym_k2": RL.unbatched_asym_norm_loss(sf_, 2, batch),
        }
        # (without a mask the padded zero rows of s would tie: the unmasked form runs on the rows every graph has)
        assert_no_quantile_tie(s[:, :4].reshape(-1, Kc), Kc, graph[:, :4].reshape(-1), "functions.nomask")
        exp["asym_nomask"] = RL.asym_norm_loss(s_[:, :4], Kc)
        CASES[f"acc_functions_{tag}"] = {
            "kind": "functions", "inputs": {"adj": a_, "s": s_, "mask": mask, "edge_index": ei, "edge_weight": ew_,
                                            "batch": batch, "s_flat": sf_},
            "expected": {k: G.t(v) for k, v in exp.items()}}


def main():
    gen_poolers()
    gen_functions()
    out = os.path.join(HERE, "golden_acc_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
