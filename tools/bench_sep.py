"""SEP pooling's selector and whole forward: the native kernel next to the host route of the same commit (the same
algorithm in float64 with a lazy heap, graph by graph: the shape of the reference's loop) and next to a
``KMISPooling(scorer="degree")`` forward on the same batch, the yardstick of a pre-coarsening pooler that is native
already.  Same timing as bench.py (median of the windows after a warm-up, device synchronised), the runs measured in
alternation inside every window round.

    python tools/bench_sep.py --workload small
    python tools/bench_sep.py --workload large

Workloads (F = 32, weighted, about 4 neighbours per node below 100 nodes and 8 above):
  small  2048 graphs of 20-60 nodes
  large  512 graphs of 100 nodes up to the kernel's node limit
The host route is timed on the first ``--subset`` graphs only (it takes milliseconds per graph) and scaled to the batch.
A new ``edge_index`` tensor is made for every call, so the selector pays for its two edge-position indices each time.
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
    ap.add_argument("--workload", choices=("small", "large"), default="small")
    ap.add_argument("--subset", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "torch-geometric-pool_amd"))
    import torch
    from tgp import kernels
    from tgp.poolers import KMISPooling, SEPPooling
    from tgp.select import sep_select

    if not torch.cuda.is_available():
        raise SystemExit("bench_sep.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    F, limit = 32, kernels.sep_max_nodes()
    if a.workload == "small":
        sizes = torch.randint(20, 61, (2048,), generator=g).tolist()
    else:
        sizes = torch.randint(100, limit + 1, (512,), generator=g).tolist()
    eis, ews, bs, off = [], [], [], 0
    for gi, n in enumerate(sizes):
        up = torch.triu(torch.rand(n, n, generator=g) < (4.0 if n < 100 else 8.0) / n, 1)
        w = torch.triu(torch.rand(n, n, generator=g) * 0.9 + 0.1, 1) * up
        adj = w + w.t()
        idx = adj.nonzero().t()
        eis.append(idx + off)
        ews.append(adj[idx[0], idx[1]])
        bs.append(torch.full((n,), gi))
        off += n
    n = off
    ei_h, ew_h, batch_h = torch.cat(eis, 1), torch.cat(ews), torch.cat(bs)
    ei, ew, batch = ei_h.to(dev), ew_h.to(dev), batch_h.to(dev)
    x = torch.randn(n, F, generator=g).to(dev)
    sub = min(a.subset, len(sizes))
    n_sub = sum(sizes[:sub])
    e_sub = int((batch_h[ei_h[0]] < sub).sum())  # (the list is grouped by graph)
    ei_s, ew_s, batch_s = ei[:, :e_sub], ew[:e_sub], batch[:n_sub]

    pool = SEPPooling()
    kmis = KMISPooling(scorer="degree")

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    runs = {
        "select": (no_grad(lambda: sep_select(ei.clone(), ew, batch)), a.steps),
        "select_indexed": (no_grad(lambda: sep_select(ei, ew, batch)), a.steps),  # the edge-position indices remembered
        "forward": (no_grad(lambda: pool(x=x, adj=ei.clone(), edge_weight=ew, batch=batch)), a.steps),
        "kmis_degree_forward": (no_grad(lambda: kmis(x=x, adj=ei.clone(), edge_weight=ew, batch=batch)), a.steps),
        "host_select_subset": (no_grad(lambda: sep_select(ei_s, ew_s, batch_s, route="host")), 1),
    }
    so = sep_select(ei, ew, batch)
    host = runs["host_select_subset"][0]()
    same = bool(torch.equal(so.cluster_index[:n_sub], host.cluster_index))
    for fn, steps in runs.values():
        for _ in range(min(a.warmup, max(1, steps))):
            fn()
    ms = {name: [] for name in runs}
    for _ in range(a.windows):
        for name, (fn, steps) in runs.items():  # alternating: every window round times each of them once
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    med = {name: statistics.median(v) for name, v in ms.items()}
    out = {"workload": a.workload, "num_graphs": len(sizes), "num_nodes": n, "num_edges": int(ei.size(1)), "features": F,
           "node_limit": limit, "largest_graph": max(sizes), "select_route": so.__dict__["_sep_route"],
           "num_supernodes": so.num_supernodes, "subset_graphs": sub, "native_equals_host_on_subset": same,
           "windows": a.windows, "steps_per_window": a.steps}
    for name in runs:
        out[f"{name}_ms_median"] = round(med[name], 5)
        out[f"{name}_ms_min"] = round(min(ms[name]), 5)
        out[f"{name}_ms_max"] = round(max(ms[name]), 5)
    out["select_ms_per_graph"] = round(med["select"] / len(sizes), 6)
    out["host_select_ms_per_graph"] = round(med["host_select_subset"] / sub, 6)
    out["host_select_ms_scaled_to_batch"] = round(med["host_select_subset"] / sub * len(sizes), 3)
    out["host_over_native_select"] = round(out["host_select_ms_scaled_to_batch"] / med["select"], 2)
    out["forward_over_kmis_degree_forward"] = round(med["forward"] / med["kmis_degree_forward"], 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
