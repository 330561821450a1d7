"""LaPool's selector and pooler: the native kernels against two composed-torch forms and against MinCut, the same inputs,
device synchronised, the candidates measured in alternation inside every window round.

    python tools/bench_lapool.py --workload sparse
    python tools/bench_lapool.py --workload dense --steps 20

Workloads:
  sparse  2048 graphs of 20-60 nodes, F = 32, an edge list: LaPooling(batched=False)
  dense   B = 32, N = 1024, F = 64, a padded adjacency (about 8 neighbours per node): LaPooling(batched=True)
Measured: the selector alone, the whole forward, forward + backward of sum(x_pool ** 2) + sum(adj_pool), and the peak
memory growth of one selector call.
Baselines:
  restatement   tests/lapool_restatement.py on device tensors: composed torch ops, graph by graph
  cross_graph   the reference-shaped composed form: the [N_total, K_total] similarity of every node against every
                leader of every graph, -inf across graphs, one softmax over all of it, then each graph's block copied
                out (one gather here; the reference loops over the graphs in Python).  Skipped above --cross-graph-gib.
  mincut        get_pooler("mincut")'s whole forward on the same batch (k = 16)
The slow baselines run steps / 10 times per window (at least once).  Prints one JSON line.
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
    ap.add_argument("--workload", choices=("sparse", "dense"), default="sparse")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cross-graph-gib", type=float, default=16.0)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "torch-geometric-pool_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import lapool_restatement as R
    from tgp.poolers import LaPooling, get_pooler
    from tgp.select import LaPoolSelect

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    sync = torch.cuda.synchronize
    if a.workload == "sparse":
        F = 32
        sizes = torch.randint(20, 61, (2048,), generator=g).tolist()
        eis, bs, off = [], [], 0
        for gi, n in enumerate(sizes):
            m = torch.triu(torch.rand(n, n, generator=g) < 4.0 / n, 1)
            eis.append((m | m.t()).nonzero().t() + off)
            bs.append(torch.full((n,), gi))
            off += n
        ei, batch = torch.cat(eis, 1).to(dev), torch.cat(bs).to(dev)
        x = torch.randn(off, F, generator=g).to(dev)
        sel, pooler = LaPoolSelect(batched_representation=False), LaPooling(batched=False)
        sel_kw, pool_kw = dict(edge_index=ei, batch=batch), dict(adj=ei, batch=batch)
        rest_kw = dict(edge_index=ei, batch=batch)
        node_graph, mask = batch, None
        shape = {"graphs": len(sizes), "num_nodes": off, "num_edges": int(ei.size(1)), "features": F}
    else:
        B, N, F = 32, 1024, 64
        up = torch.triu(torch.rand(B, N, N, generator=g) < 8.0 / N, 1).float()
        adj = (up + up.transpose(1, 2)).to(dev)
        x = torch.randn(B, N, F, generator=g).to(dev)
        sel, pooler = LaPoolSelect(), LaPooling()
        sel_kw, pool_kw, rest_kw = dict(edge_index=adj), dict(adj=adj), dict(adj=adj)
        node_graph, mask = torch.arange(B, device=dev).repeat_interleave(N), None
        shape = {"graphs": B, "nodes_per_graph": N, "features": F}
    mincut = get_pooler("mincut", in_channels=F, k=16, batched=a.workload == "dense").to(dev).eval()

    with torch.no_grad():
        so = sel(x, **sel_kw)
    leaders = so.leader_mask
    k_total, k_max = int(leaders.sum()), so.s.size(-1)
    n_total = leaders.numel()
    cross_bytes = n_total * k_total * 4
    xf, lf = x.reshape(n_total, -1), leaders.reshape(-1)

    def native_select():
        with torch.no_grad():
            return sel(x, **sel_kw).s

    def restatement():
        with torch.no_grad():
            return R.select(x, **rest_kw)[2]

    def cross_graph():
        # the leader set comes from the restatement's first two steps; the assignment is the reference-shaped one
        with torch.no_grad():
            v = R.variation(x, rest_kw.get("adj"), mask, edge_index=rest_kw.get("edge_index"))
            lead = R.leaders_from(v, rest_kw.get("adj"), mask, edge_index=rest_kw.get("edge_index"),
                                  batch=rest_kw.get("batch")).reshape(-1)
            idx = lead.nonzero(as_tuple=True)[0]
            xl = xf[idx]
            sim = (xf @ xl.t()) / (xf.norm(dim=-1, keepdim=True) * xl.norm(dim=-1, keepdim=True).t() + 1e-8)
            sim = sim.masked_fill(node_graph.unsqueeze(1) != node_graph[idx].unsqueeze(0), float("-inf"))
            s = torch.softmax(sim, dim=-1)
            s[idx] = 0.0
            s[idx, torch.arange(idx.numel(), device=dev)] = 1.0
            kb = torch.bincount(node_graph[idx], minlength=int(node_graph.max()) + 1)
            start = torch.cumsum(kb, 0) - kb
            cols = start[node_graph].unsqueeze(1) + torch.arange(int(kb.max()), device=dev).unsqueeze(0)
            ok = torch.arange(int(kb.max()), device=dev).unsqueeze(0) < kb[node_graph].unsqueeze(1)
            return torch.gather(s, 1, cols.clamp_max(idx.numel() - 1)) * ok

    def forward():
        with torch.no_grad():
            return pooler(x=x, **pool_kw)

    def forward_backward():
        leaf = x.detach().requires_grad_(True)
        out = pooler(x=leaf, **pool_kw)
        loss = (out.x ** 2).sum() + (out.edge_weight if out.edge_weight is not None else out.edge_index).sum()
        loss.backward()
        return leaf.grad

    def mincut_forward():
        with torch.no_grad():
            return mincut(x=x, **pool_kw)

    runs = {"native_select": (native_select, 1), "restatement": (restatement, 10), "lapool_forward": (forward, 1),
            "lapool_forward_backward": (forward_backward, 1), "mincut_forward": (mincut_forward, 1)}
    if cross_bytes <= a.cross_graph_gib * 2 ** 30:
        runs["cross_graph"] = (cross_graph, 10)
    same_leaders = bool(torch.equal(R.select(x, **rest_kw)[1].reshape(-1), lf))
    err = float((native_select() - restatement()).abs().max())
    if "cross_graph" in runs and same_leaders:
        err = max(err, float((native_select().reshape(n_total, -1) - cross_graph()).abs().max()))
    for fn, slow in runs.values():
        for _ in range(max(1, a.warmup // slow)):
            fn()
    ms = {name: [] for name in runs}
    for _ in range(a.windows):
        for name, (fn, slow) in runs.items():
            steps = max(1, a.steps // slow)
            sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            sync()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    peak = {}
    for name in ("native_select", "restatement", "cross_graph"):
        if name in runs:
            sync()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            runs[name][0]()
            sync()
            peak[name] = torch.cuda.max_memory_allocated() - before
    out = {"workload": a.workload, **shape, "k_total": k_total, "k_max": k_max, "cross_graph_matrix_bytes": cross_bytes,
           "leaders_equal_restatement": same_leaders, "max_abs_s_difference": err, "windows": a.windows,
           "steps_per_window": a.steps,
           # variation, flags, columns (+ the memset of its K_max word), the count's publish, row norms, assignment;
           # the edge form adds the by-source index build in front
           "select_own_launches_per_call": 6}
    for name in runs:
        out[f"{name}_ms_median"] = round(statistics.median(ms[name]), 5)
        out[f"{name}_ms_min"] = round(min(ms[name]), 5)
        out[f"{name}_ms_max"] = round(max(ms[name]), 5)
    for name, b in peak.items():
        out[f"{name}_peak_bytes"] = int(b)
    out["native_over_restatement"] = round(out["native_select_ms_median"] / out["restatement_ms_median"], 5)
    out["lapool_forward_over_mincut_forward"] = round(out["lapool_forward_ms_median"] / out["mincut_forward_ms_median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
