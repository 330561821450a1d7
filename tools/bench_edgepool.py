"""Edge-contraction selection and pooling: the native kernels against the composed-torch restatement and against
Graclus, the same inputs, the same timing as bench.py (median of 5 windows after a warm-up, device synchronised), all of
them measured in alternation inside every window round.

    python tools/bench_edgepool.py --workload small
    python tools/bench_edgepool.py --workload large --steps 5 --warmup 2

Workloads:
  small  2048 graphs of 20-60 nodes, F = 32, softmax scores
  large  one graph, N = 1M, E = 10M entries, F = 128, softmax scores
Timed:
  native_scores    kernels.edge_contract_scores (projection, raw scores, by-destination index, softmax)
  native_matching  kernels.edge_contract_select behind those scores (matching, relabelling, weights)
  native_select    the whole EdgeContractionSelect forward (both of the above + the SelectOutput)
  restatement      tests/edgepool_restatement.py on device tensors: the reference's algorithm as composed torch ops (scores,
                   stable argsort, rounds with one host read each, clusters, weights)
  forward          the whole EdgeContractionPooling forward
  graclus_forward  get_pooler("graclus")'s whole forward on the same batch

Bytes counted, the streams a kernel cannot avoid (gathered operands and atomics are not counted, so the shares are
lower bounds on the traffic):
  scores  x once (4 N F) + the two projections written (8 N); per entry the indices (16 B) and the raw score written
          (4 B); the statistics pass' index and two gathered reads of raw (4 + 8 B), 8 B per node written; the apply pass'
          raw, target and result (4 + 8 + 4 B)
  round   push: 16 B of indices per entry; decide: 16 B per entry + 8 B per node reset
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
    ap.add_argument("--method", choices=("softmax", "tanh", "sigmoid"), default="softmax")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "torch-geometric-pool_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import edgepool_restatement as R
    from tgp import kernels
    from tgp.poolers import EdgeContractionPooling, get_pooler
    from tgp.select import EdgeContractionSelect
    from tgp.utils.ops import batch_info

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
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
    else:
        F = 128
        n, e = 1_000_000, 10_000_000
        half = torch.randint(0, n, (2, e // 2), generator=g)
        ei = torch.cat([half, half.flip(0)], 1)
        ei = ei[:, torch.sort(ei[0], stable=True)[1]].contiguous().to(dev)
        batch = None
    E = int(ei.size(1))
    x = torch.randn(n, F, generator=g).to(dev)
    method = getattr(EdgeContractionSelect, "compute_edge_score_" + a.method)
    pooler = EdgeContractionPooling(in_channels=F, edge_score_method=method).to(dev).eval()
    graclus = get_pooler("graclus").to(dev).eval()
    sel = pooler.selector
    w, b = sel.lin.weight.detach(), sel.lin.bias.detach()
    gptr = gmax = None
    if batch is not None:
        info = batch_info(batch)
        gptr, gmax = info.ptr, info.max_nodes

    def native_scores():
        return kernels.edge_contract_scores(x, ei, w, b, a.method, 0.5)

    score = native_scores()

    def native_matching():
        return kernels.edge_contract_select(ei, n, score, graph_ptr=gptr, max_graph_nodes=gmax)

    def native_select():
        with torch.no_grad():
            return sel(x, ei, batch=batch)

    def restatement():
        e = R.scores(x, ei, w, b, a.method, 0.5)
        return R.select(e, ei, n)

    def forward():
        with torch.no_grad():
            return pooler(x=x, adj=ei, batch=batch)

    def graclus_forward():
        with torch.no_grad():
            return graclus(x=x, adj=ei, batch=batch)

    runs = {"native_scores": native_scores, "native_matching": native_matching, "native_select": native_select,
            "restatement": restatement, "forward": forward, "graclus_forward": graclus_forward}
    res = native_matching()
    match_ref, rounds_ref = R.matching(ei, n, R.stable_perm(score), return_rounds=True)
    cluster_ref, k_ref = R.clusters(ei, n, match_ref)
    same = bool(torch.equal(res.matched.bool(), match_ref) and torch.equal(res.index[1], cluster_ref) and res.k == k_ref)
    e_ref = R.scores(x.double(), ei, w.double(), b.double(), a.method, 0.5)
    score_err = float((score.double() - e_ref).abs().max())
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
    out = {"workload": a.workload, "method": a.method, "num_nodes": n, "num_edges": E, "features": F, "route": res.route,
           "supernodes": res.k, "matched_entries": int(match_ref.sum()), "rounds_needed": rounds_ref,
           "rounds_native": res.rounds, "equals_restatement": same, "score_max_abs_err_vs_float64": score_err,
           "windows": a.windows, "steps_per_window": a.steps}
    for name in runs:
        out[f"{name}_ms_median"] = round(med[name], 5)
        out[f"{name}_ms_min"] = round(min(ms[name]), 5)
        out[f"{name}_ms_max"] = round(max(ms[name]), 5)
    out["native_select_over_restatement"] = round(med["native_select"] / med["restatement"], 4)
    out["forward_over_graclus_forward"] = round(med["forward"] / med["graclus_forward"], 4)
    score_bytes = 4 * n * F + 8 * n + 20 * E
    if a.method == "softmax":
        score_bytes += 12 * E + 8 * n + 16 * E
    else:
        score_bytes += 8 * E
    out["score_bytes_counted"] = score_bytes
    out["scores_share_of_hbm_peak"] = round(score_bytes / (med["native_scores"] * 1e-3) / HBM_PEAK, 4)
    if res.route == "graphs":
        out["matching_host_waits_per_call"] = 1  # status, rounds and the cluster count in one read
        out["matching_launches_per_call"] = 4  # the per-graph kernel, two relabel kernels, the weights (+ 2 memsets)
    else:
        # the flags are read after 4, 12, 28, ... rounds; then the cluster count
        launched, step, waits = 0, 4, 0
        while launched < res.rounds + 1:
            launched += step
            step = min(2 * step, 256)
            waits += 1
        out["rounds_launched"] = launched
        out["matching_host_waits_per_call"] = waits + 1
        out["matching_launches_per_call"] = 1 + 2 * launched + 3  # init, two per round, two relabel kernels, the weights
        round_bytes = 32 * E + 8 * n
        round_ms = med["native_matching"] / launched
        out["ms_per_round_mean"] = round(round_ms, 5)
        out["round_bytes_counted"] = round_bytes
        out["round_share_of_hbm_peak"] = round(round_bytes / (round_ms * 1e-3) / HBM_PEAK, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
