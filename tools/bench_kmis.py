"""k-MIS selection and pooling: the native kernels against the composed-torch restatement and against Graclus, the same
inputs, the same timing as bench.py (median of 5 windows of 200 steps after a warm-up, device synchronised), the three
measured in alternation inside every window round.

    python tools/bench_kmis.py --workload small --order-k 1
    python tools/bench_kmis.py --workload large --steps 5

Workloads:
  small  2048 graphs of 20-60 nodes, F = 32, linear scorer, "greedy": the selector alone (kernels.kmis_select behind the
         score), the whole KMISPooling forward, launches per call, rounds taken
  large  one graph, N = 1M, E = 10M: the selector alone, rounds taken, ms per hop and the hop kernel's share of HBM peak
Baselines:
  restatement  tests/kmis_restatement.py on device tensors: the reference's algorithm as composed torch ops, one host
               read per round included
  graclus      get_pooler("graclus")'s whole forward on the same batch

Bytes counted for a hop (device-wide route): the streams a hop cannot avoid -- 16 B of indices per edge, and per node the
own value read, the destination written and the third buffer reset (24 B for a min hop, 3 B for a mask hop); the
gathers of source values and the atomics are not counted, so the share is a lower bound on the traffic.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12  # bytes / s, MI355X


def _sync():
    import torch
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("small", "large"), default="small")
    ap.add_argument("--order-k", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "torch-geometric-pool_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import kmis_restatement as R
    from tgp import kernels
    from tgp.poolers import KMISPooling, get_pooler
    from tgp.utils.ops import batch_info

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    k, F = a.order_k, 32
    if a.workload == "small":
        sizes = torch.randint(20, 61, (2048,), generator=g).tolist()
        eis, bs, off = [], [], 0
        for gi, n in enumerate(sizes):
            m = torch.triu(torch.rand(n, n, generator=g) < 4.0 / n, 1)
            eis.append((m | m.t()).nonzero().t() + off)
            bs.append(torch.full((n,), gi))
            off += n
        ei, batch, n = torch.cat(eis, 1).to(dev), torch.cat(bs).to(dev), off
    else:
        n, e = 1_000_000, 10_000_000
        half = torch.randint(0, n, (2, e // 2), generator=g)
        ei = torch.cat([half, half.flip(0)], 1)
        ei = ei[:, torch.sort(ei[0], stable=True)[1]].contiguous().to(dev)
        batch = None
    x = torch.randn(n, F, generator=g).to(dev)
    pooler = KMISPooling(in_channels=F, order_k=k).to(dev).eval()
    graclus = get_pooler("graclus").to(dev).eval()
    with torch.no_grad():
        score = pooler.selector.lin(x).sigmoid().view(-1)
    gptr = gmax = None
    if batch is not None:
        info = batch_info(batch)
        gptr, gmax = info.ptr, info.max_nodes

    def native_select():
        return kernels.kmis_select(ei, n, k, score=score, heuristic="greedy", graph_ptr=gptr, max_graph_nodes=gmax)

    def restatement():
        return R.select(score, ei, k, "greedy", n)

    def forward():
        with torch.no_grad():
            return pooler(x=x, adj=ei, batch=batch)

    def graclus_forward():
        with torch.no_grad():
            return graclus(x=x, adj=ei, batch=batch)

    runs = {"native_select": native_select, "restatement": restatement, "kmis_forward": forward,
            "graclus_forward": graclus_forward}
    res = native_select()
    mis_ref, cluster_ref, _ = restatement()
    same = bool(torch.equal(res.mis, mis_ref) and torch.equal(res.index[1], cluster_ref))
    _, _, rounds_ref = R.mis_cluster(ei, k, R.stable_perm(res.updated), n, return_rounds=True)
    for fn in runs.values():
        for _ in range(min(a.warmup, max(2, a.steps))):
            fn()
    ms = {name: [] for name in runs}
    for _ in range(a.windows):
        for name, fn in runs.items():  # alternating: every window round times each of them once
            _sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            _sync()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    med = {name: statistics.median(v) for name, v in ms.items()}
    out = {"workload": a.workload, "order_k": k, "num_nodes": n, "num_edges": int(ei.size(1)), "route": res.route,
           "supernodes": res.k, "rounds_needed": rounds_ref, "rounds_launched": res.rounds,
           "equals_restatement": same, "windows": a.windows, "steps_per_window": a.steps}
    for name in runs:
        out[f"{name}_ms_median"] = round(med[name], 5)
        out[f"{name}_ms_min"] = round(min(ms[name]), 5)
        out[f"{name}_ms_max"] = round(max(ms[name]), 5)
    out["native_over_restatement"] = round(med["native_select"] / med["restatement"], 4)
    out["kmis_forward_over_graclus_forward"] = round(med["kmis_forward"] / med["graclus_forward"], 4)
    if res.route == "graphs":
        # the per-graph kernel (+ the memset of its status word), two relabel kernels, the member list
        out["select_launches_per_call"] = 5
    else:
        # per round 2k hops; the cluster pass k hops + the owners; the "greedy" counts k hops + the division; the keys;
        # two relabel kernels and the member list (memsets not counted)
        hops = res.rounds * 2 * k + k
        out["select_launches_per_call"] = hops + 1 + k + 1 + 1 + 3
        E = int(ei.size(1))
        hop_ms = med["native_select"] / (hops + k)
        min_bytes, mask_bytes = 16 * E + 24 * n, 16 * E + 3 * n
        out["ms_per_hop_mean"] = round(hop_ms, 5)
        out["hop_bytes_counted_min_hop"] = min_bytes
        out["hop_bytes_counted_mask_hop"] = mask_bytes
        out["hop_share_of_hbm_peak"] = round((min_bytes + mask_bytes) / 2 / (hop_ms * 1e-3) / HBM_PEAK, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
