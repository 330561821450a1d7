"""SAGPooling's scorer and whole forward: the native project-then-aggregate kernels against the composed device form
(gather, ``index_add_``, two ``Linear``s) and against TopkPooling's forward, the same inputs, the same timing as bench.py
(median of 5 windows after a warm-up, device synchronised), all of them measured in alternation inside every window
round.

    python tools/bench_sag.py --workload small
    python tools/bench_sag.py --workload large --steps 10 --warmup 3

Workloads:
  small  2048 graphs of 20-60 nodes, F = 32
  large  one graph, N = 1M, E = 10M entries, F = 128
Timed:
  native_scorer    GraphConv.score: row_project2 + the aggregate with tanh fused (the by-destination index remembered)
  native_project   kernels.row_project2 alone: the one pass over x
  native_aggregate kernels.sag_aggregate alone: the E scalar gathers
  row_dot_twice    kernels.row_dot called twice: what row_project2 has to beat
  topk_score       kernels.topk_score on the same x: the rate of the existing one-projection pass
  index_build      kernels.sag_edge_group with the memo cleared: what a NEW edge list pays once
  composed_scorer  tanh(lin_rel(zeros.index_add_(dst, x[src])) + lin_root(x)) as ATen ops on the device
  forward          the whole SAGPooling forward
  topk_forward     TopkPooling's whole forward on the same batch
Bytes counted (the streams a kernel cannot avoid; gathered operands are not counted, so the shares are lower bounds):
  project    x once (4 N F) + two vectors written (8 N)
  aggregate  offsets (4 N), positions (4 E, the permutation route) and source ids (8 E), q read and a written (8 N)
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "torch-geometric-pool_amd"))
    import torch
    from tgp import kernels
    from tgp.poolers import SAGPooling, TopkPooling

    if not torch.cuda.is_available():
        raise SystemExit("bench_sag.py measures on the GPU: none found")
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
    sag = SAGPooling(in_channels=F).to(dev).eval()
    topk = TopkPooling(in_channels=F).to(dev).eval()
    rel, root = sag.gnn.lin_rel, sag.gnn.lin_root
    w_rel, w_root, bias = rel.weight.detach(), root.weight.detach(), rel.bias.detach()
    w_topk = topk.selector.weight.detach()
    grp = kernels.sag_edge_group(ei, n)
    p, q = kernels.row_project2(x, w_rel, w_root)

    def native_scorer():
        with torch.no_grad():
            return sag.gnn.score(x, ei, True)

    def native_project():
        return kernels.row_project2(x, w_rel, w_root)

    def native_aggregate():
        return kernels.sag_aggregate(grp, ei[0], p, q, bias, tanh=True)

    def row_dot_twice():
        return kernels.row_dot(x, w_rel), kernels.row_dot(x, w_root)

    def topk_score():
        return kernels.topk_score(x, w_topk, True)

    def index_build():
        kernels._SAG_GROUPS.clear()
        return kernels.sag_edge_group(ei, n)

    def composed_scorer():
        with torch.no_grad():
            agg = torch.zeros_like(x).index_add_(0, ei[1], x[ei[0]])
            return torch.tanh(rel(agg) + root(x)).view(-1)

    def forward():
        with torch.no_grad():
            return sag(x=x, adj=ei, batch=batch)

    def topk_forward():
        with torch.no_grad():
            return topk(x=x, adj=ei, batch=batch)

    runs = {"native_scorer": native_scorer, "native_project": native_project, "native_aggregate": native_aggregate,
            "row_dot_twice": row_dot_twice, "topk_score": topk_score, "index_build": index_build,
            "composed_scorer": composed_scorer, "forward": forward, "topk_forward": topk_forward}
    with torch.no_grad():
        want = torch.tanh((torch.zeros(n, F, dtype=torch.float64, device=dev).index_add_(0, ei[1], x.double()[ei[0]])
                           @ w_rel.double().view(-1)) + bias.double() + x.double() @ w_root.double().view(-1))
    err_native = float((native_scorer().double() - want).abs().max())
    err_composed = float((composed_scorer().double() - want).abs().max())
    del want
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
    out = {"workload": a.workload, "num_nodes": n, "num_edges": E, "features": F,
           "index_route": "offsets" if grp.perm is None else "permutation",
           "supernodes": int(forward().so.num_supernodes), "native_max_abs_err_vs_float64": err_native,
           "composed_max_abs_err_vs_float64": err_composed, "windows": a.windows, "steps_per_window": a.steps}
    for name in runs:
        out[f"{name}_ms_median"] = round(med[name], 5)
        out[f"{name}_ms_min"] = round(min(ms[name]), 5)
        out[f"{name}_ms_max"] = round(max(ms[name]), 5)
    out["native_scorer_over_composed"] = round(med["native_scorer"] / med["composed_scorer"], 4)
    out["project_over_row_dot_twice"] = round(med["native_project"] / med["row_dot_twice"], 4)
    out["project_over_topk_score"] = round(med["native_project"] / med["topk_score"], 4)
    out["forward_over_topk_forward"] = round(med["forward"] / med["topk_forward"], 4)
    project_bytes = 4 * n * F + 8 * n
    aggregate_bytes = 4 * n + (4 * E if grp.perm is not None else 0) + 8 * E + 8 * n
    out["project_bytes_counted"] = project_bytes
    out["project_share_of_hbm_peak"] = round(project_bytes / (med["native_project"] * 1e-3) / HBM_PEAK, 4)
    out["topk_score_share_of_hbm_peak"] = round((4 * n * F + 4 * n) / (med["topk_score"] * 1e-3) / HBM_PEAK, 4)
    out["aggregate_bytes_counted"] = aggregate_bytes
    out["aggregate_share_of_hbm_peak"] = round(aggregate_bytes / (med["native_aggregate"] * 1e-3) / HBM_PEAK, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
