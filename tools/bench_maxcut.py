"""MaxCutPooling's three native parts and whole forward: each against the composed device form on the same inputs, the
forward next to TopkPooling's and SAGPooling's, and a training step; the same timing as bench.py (median of 5 windows
after a warm-up, device synchronised), all measured in alternation inside every window round.

    python tools/bench_maxcut.py --workload small
    python tools/bench_maxcut.py --workload large --steps 5 --warmup 2
    python tools/bench_maxcut.py --workload hub --steps 2 --warmup 1
    python tools/bench_maxcut.py --workload hub_sweep --steps 10 --warmup 2

Workloads:
  small  2048 graphs of 20-60 nodes, F = 32
  large  one graph, N = 1M, E = 10M entries, F = 128
  hub    one graph, N = 65536, 524288 random edges and ONE node with 524288 more in-edges (in-degree 524295), F = 128:
         the hub's groups take the chunked route of csrc/maxcut_hub.hip (kernels_score: the one-wave kernels with
         the plan suppressed and the gate off, as before that route)
  hub_sweep  the hub list with in-degrees 1024 .. 524295 (--degrees), a JSON line each: see hub_sweep()
Timed (the by-destination / by-source indices and n_P are remembered per edge list, as in full-batch training):
  native_score / composed_score     MaxCutScoreNet (pooler default: 4 layers of 32) without grad, as the class routes it /
                                    the composed form
  kernels_score                     the score net's one-wave kernels: the hub gate switched off, the hub plan suppressed
  native_loss / composed_loss       the cut loss of the scores
  native_assign / composed_assign   the nearest-supernode assignment of the same top-k selection (max_iter = 5)
  forward / composed_forward        the whole MaxCutPooling forward (inference); composed: score net, loss and assignment
                                    as ATen ops, Reduce and Connect the same
  topk_forward, sag_forward         TopkPooling's and SAGPooling's forwards on the same batch
  train_step / composed_train       forward + backward of sum(x_pool^2) + loss through the native nodes / the ATen ops
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("small", "large", "hub", "hub_sweep"), default="small")
    ap.add_argument("--degrees", type=int, nargs="*", default=[1024, 4096, 16384, 65536, 524295],
                    help="hub_sweep: the in-degrees of the one hub, a JSON line each")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--one-wave-steps", type=int, default=1, help="hub_sweep: steps per window of the one-wave forms")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "torch-geometric-pool_amd"))
    import torch
    from tgp import kernels
    from tgp.poolers import MaxCutPooling, SAGPooling, TopkPooling
    from tgp.select import TopkSelect
    from tgp.utils import losses as L

    if not torch.cuda.is_available():
        raise SystemExit("bench_maxcut.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if a.workload == "hub_sweep":
        return hub_sweep(a, torch, kernels, MaxCutPooling, TopkSelect, L, dev)
    g = torch.Generator().manual_seed(0)
    batch = None
    if a.workload == "small":
        F = 32
        sizes = torch.randint(20, 61, (2048,), generator=g).tolist()
        eis, bs, off = [], [], 0
        for gi, n in enumerate(sizes):
            m = torch.triu(torch.rand(n, n, generator=g) < 4.0 / n, 1)
            eis.append((m | m.t()).nonzero().t() + off)
            bs.append(torch.full((n,), gi))
            off += n
        ei, batch, n = torch.cat(eis, 1).to(dev), torch.cat(bs).to(dev), off
    elif a.workload == "large":
        F = 128
        n, e = 1_000_000, 10_000_000
        half = torch.randint(0, n, (2, e // 2), generator=g)
        ei = torch.cat([half, half.flip(0)], 1)
        ei = ei[:, torch.sort(ei[0], stable=True)[1]].contiguous().to(dev)
    else:
        F = 128
        n, e = 65536, 524288
        ei = torch.cat([torch.randint(0, n, (2, e), generator=g),
                        torch.stack([torch.randint(0, n, (e,), generator=g), torch.full((e,), 7)])], 1).to(dev)
    x = torch.randn(n, F, generator=g).to(dev)
    # (no batch vector: Connect cannot normalise the pooled weights per graph, as in the reference)
    pool = MaxCutPooling(in_channels=F, edge_weight_norm=batch is not None).to(dev).eval()
    sag = SAGPooling(in_channels=F).to(dev).eval()
    topk = TopkPooling(in_channels=F).to(dev).eval()
    sel, net = pool.selector, pool.selector.score_net

    class composed:
        """Inside: the score net, the loss and the assignment take their composed device forms."""

        def __enter__(self):
            self.saved = (net.native_case, L.maxcut_loss_native_case, sel.assign)
            net.native_case = lambda *args: False
            L.maxcut_loss_native_case = lambda *args: False
            sel.assign = lambda so, edge_index, weight, b, max_iter=None: so.assign_all_nodes(
                adj=edge_index, weight=weight, max_iter=sel.max_iter if max_iter is None else max_iter, batch=b,
                closest_node_assignment=True)

        def __exit__(self, *exc):
            net.native_case, L.maxcut_loss_native_case = self.saved[0], self.saved[1]
            del sel.assign

    with torch.no_grad():
        scores = net(x, ei).view(-1)
        so_topk = TopkSelect.forward(sel, x=scores.view(-1, 1), batch=batch)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def in_composed(fn):
        def run():
            with composed():
                return fn()
        return run

    def with_kernels(fn):
        def run():
            gate = kernels.maxcut_score_has_hub
            kernels.maxcut_score_has_hub = lambda *args: False
            idx = [kernels.sag_edge_group(ei, n, by_destination=b) for b in (True, False)]
            plans = [i.hub for i in idx]
            for i in idx:
                i.hub = None
            try:
                return fn()
            finally:
                kernels.maxcut_score_has_hub = gate
                for i, plan in zip(idx, plans):
                    i.hub = plan
        return run

    def step():
        pool.zero_grad(set_to_none=True)
        xg = x.detach().requires_grad_(True)
        out = pool(x=xg, adj=ei, batch=batch)
        ((out.x ** 2).sum() + out.loss["maxcut_loss"]).backward()

    runs = {
        "native_score": no_grad(lambda: net(x, ei)),
        "kernels_score": no_grad(with_kernels(lambda: net(x, ei))),
        "composed_score": no_grad(in_composed(lambda: net(x, ei))),
        "native_loss": no_grad(lambda: L.maxcut_loss(scores, ei, None, batch)),
        "composed_loss": no_grad(in_composed(lambda: L.maxcut_loss(scores, ei, None, batch))),
        "native_assign": no_grad(lambda: sel.assign(so_topk, ei, scores, batch)),
        "composed_assign": no_grad(in_composed(lambda: sel.assign(so_topk, ei, scores, batch))),
        "forward": no_grad(lambda: pool(x=x, adj=ei, batch=batch)),
        "composed_forward": no_grad(in_composed(lambda: pool(x=x, adj=ei, batch=batch))),
        "topk_forward": no_grad(lambda: topk(x=x, adj=ei, batch=batch)),
        "sag_forward": no_grad(lambda: sag(x=x, adj=ei, batch=batch)),
        "train_step": step,
        "composed_train": in_composed(step),
    }
    torch.manual_seed(1)
    nat = runs["forward"]()
    torch.manual_seed(1)
    comp = runs["composed_forward"]()
    err = {"scores": float((nat.so.scores.double() - comp.so.scores.double()).abs().max()),
           "loss": float((nat.loss["maxcut_loss"].double() - comp.loss["maxcut_loss"].double()).abs()),
           "same_assignment": bool(torch.equal(nat.so.cluster_index, comp.so.cluster_index))}
    supernodes = int(nat.so.num_supernodes)
    del nat, comp
    for fn in runs.values():
        for _ in range(min(a.warmup, max(2, a.steps))):
            fn()
    ms = {name: [] for name in runs}
    for _ in range(a.windows):
        for name, fn in runs.items():  # alternating: every window round times each of them once
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    med = {name: statistics.median(v) for name, v in ms.items()}
    grp = kernels.sag_edge_group(ei, n)
    out = {"workload": a.workload, "num_nodes": n, "num_edges": int(ei.size(1)), "features": F,
           "index_route": "offsets" if grp.perm is None else "permutation",
           "max_in_degree": int((grp.row_ptr[1:] - grp.row_ptr[:-1]).max()), "supernodes": supernodes,
           "hubs": 0 if grp.hub is None else grp.hub.H, "hub_chunks": 0 if grp.hub is None else grp.hub.chunks,
           "score_route": "composed (hub gate)" if kernels.maxcut_score_has_hub(ei, n) else "kernels",
           "windows": a.windows, "steps_per_window": a.steps, "native_vs_composed": err}
    for name in runs:
        out[f"{name}_ms_median"] = round(med[name], 5)
        out[f"{name}_ms_min"] = round(min(ms[name]), 5)
        out[f"{name}_ms_max"] = round(max(ms[name]), 5)
    out["kernels_score_over_composed"] = round(med["kernels_score"] / med["composed_score"], 4)
    for part in ("score", "loss", "assign"):
        out[f"native_{part}_over_composed"] = round(med[f"native_{part}"] / med[f"composed_{part}"], 4)
    out["forward_over_composed_forward"] = round(med["forward"] / med["composed_forward"], 4)
    out["train_step_over_composed_train"] = round(med["train_step"] / med["composed_train"], 4)
    out["forward_over_sag_forward"] = round(med["forward"] / med["sag_forward"], 4)
    out["forward_over_topk_forward"] = round(med["forward"] / med["topk_forward"], 4)
    print(json.dumps(out))


def hub_sweep(a, torch, kernels, MaxCutPooling, TopkSelect, L, dev):
    """One JSON line per hub in-degree: 65536 nodes, 524288 random edges and ``degree`` more into node 7, F = 128 (the
    hub's sources see it as a by-source hub in the backward only through the random edges: the by-source index has no
    hub).  The same list as two tensor objects: the index of one is built with the plan suppressed and runs with both
    gates off (the one-wave kernels), the index of the other with the threshold just below the degree (the hub route,
    whatever HUB_MIN_GROUP is); the composed form runs on the first.  One run times the three forms in alternating
    windows: the score net without grad, its forward + backward, the assignment rounds (max_iter = 5) of one top-k
    selection, the whole forward and the training step.  The one-wave assignment walks a group once per distinct label,
    so it (and the one-wave forward and step, which contain it) is timed up to HUB_MIN_GROUP only, the bound the gate
    before the hub route refused above; the one-wave forms run ``--one-wave-steps`` steps per window."""
    F, n, e = 128, 65536, 524288
    pool = MaxCutPooling(in_channels=F, edge_weight_norm=False).to(dev).eval()
    sel, net = pool.selector, pool.selector.score_net
    shipped = kernels.HUB_MIN_GROUP

    class composed:
        def __enter__(self):
            self.saved = (net.native_case, L.maxcut_loss_native_case)
            net.native_case = lambda *args: False
            L.maxcut_loss_native_case = lambda *args: False
            sel.assign = lambda so, edge_index, weight, b, max_iter=None: so.assign_all_nodes(
                adj=edge_index, weight=weight, max_iter=sel.max_iter if max_iter is None else max_iter, batch=b,
                closest_node_assignment=True)

        def __exit__(self, *exc):
            net.native_case, L.maxcut_loss_native_case = self.saved
            del sel.assign

    class gates_off:
        def __enter__(self):
            self.saved = (kernels.maxcut_score_has_hub, kernels.MAXCUT_ASSIGN_MAX_GROUP)
            kernels.maxcut_score_has_hub, kernels.MAXCUT_ASSIGN_MAX_GROUP = (lambda *args: False), 1 << 40

        def __exit__(self, *exc):
            kernels.maxcut_score_has_hub, kernels.MAXCUT_ASSIGN_MAX_GROUP = self.saved

    class as_shipped:
        def __enter__(self):
            pass

        def __exit__(self, *exc):
            pass

    for degree in a.degrees:
        g = torch.Generator().manual_seed(0)
        ei = torch.cat([torch.randint(0, n, (2, e), generator=g),
                        torch.stack([torch.randint(0, n, (degree,), generator=g), torch.full((degree,), 7)])], 1).to(dev)
        x = torch.randn(n, F, generator=g).to(dev)
        lists = {"one_wave": ei, "hub_route": ei.clone(), "composed": ei}
        ctx = {"one_wave": gates_off, "hub_route": as_shipped, "composed": composed}
        kernels.HUB_MIN_GROUP = 1 << 40  # the first sight of a list builds its indices: here without a plan
        with torch.no_grad(), gates_off():
            scores = net(x, ei).view(-1)
            so_topk = TopkSelect.forward(sel, x=scores.view(-1, 1), batch=None)
        kernels.HUB_MIN_GROUP = min(degree - 1, shipped)
        with torch.no_grad():
            net(x, lists["hub_route"])  # ... and here with one
        kernels.HUB_MIN_GROUP = shipped
        plans = {k: kernels.sag_edge_group(v, n).hub for k, v in lists.items()}
        assert plans["one_wave"] is None and plans["hub_route"] is not None and plans["hub_route"].H >= 1

        def score(k):
            with torch.no_grad(), ctx[k]():
                return net(x, lists[k])

        def train(k):
            pool.zero_grad(set_to_none=True)
            xg = x.detach().requires_grad_(True)
            with ctx[k]():
                (net(xg, lists[k]).view(-1) ** 2).sum().backward()

        def assign(k):
            with torch.no_grad(), ctx[k]():
                return sel.assign(so_topk, lists[k], scores, None)

        def forward(k):
            with torch.no_grad(), ctx[k]():
                return pool(x=x, adj=lists[k])

        def step(k):
            pool.zero_grad(set_to_none=True)
            xg = x.detach().requires_grad_(True)
            with ctx[k]():
                out = pool(x=xg, adj=lists[k])
                ((out.x ** 2).sum() + out.loss["maxcut_loss"]).backward()

        runs = {}
        for k in lists:
            parts = {"score": score, "score_train": train, "assign": assign, "forward": forward, "train_step": step}
            if k == "one_wave" and degree > shipped:
                parts = {"score": score, "score_train": train}
            runs.update({f"{k}_{part}": (lambda fn=fn, k=k: fn(k)) for part, fn in parts.items()})
        steps = {name: a.one_wave_steps if name.startswith("one_wave") else a.steps for name in runs}
        for name, fn in runs.items():
            for _ in range(max(1, min(a.warmup, steps[name]))):
                fn()
        torch.manual_seed(1)  # (the leftovers of the rounds are drawn at random)
        a_hub = assign("hub_route")
        torch.manual_seed(1)
        a_comp = assign("composed")
        ms = {name: [] for name in runs}
        for _ in range(a.windows):
            for name, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps[name]):
                    fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / steps[name] * 1e3)
        out = {"workload": "hub_sweep", "hub_in_degree": degree, "num_nodes": n, "features": F,
               "chunk": kernels.hub_chunk(), "hubs": plans["hub_route"].H, "hub_chunks": plans["hub_route"].chunks,
               "hub_is_kept": bool((so_topk.node_index == 7).any()),  # (a kept node's rounds have nothing to count)
               "windows": a.windows, "steps_per_window": a.steps, "one_wave_steps_per_window": a.one_wave_steps,
               "score_err_hub_vs_composed": float((score("hub_route").double() - score("composed").double()).abs().max()),
               "same_assignment": bool(torch.equal(a_hub.cluster_index, a_comp.cluster_index))}
        for name, v in ms.items():
            out[f"{name}_ms"] = [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]  # median, min, max
        print(json.dumps(out), flush=True)
        kernels._SAG_GROUPS.clear()


if __name__ == "__main__":
    main()
