"""DMoN against MinCut: the same inputs, the same timing as bench.py (median of 5 windows of 200 steps).

    python tools/bench_dmon.py --pooler dmon   --workload c2          # this tree
    python tools/bench_dmon.py --pooler mincut --workload c2 --tree DIR  # another checkout (e.g. the parent commit)

Workloads:
  c2        dense padded inference, B = 32 graphs x N = 1024 nodes, K = 128, F = 64 (adjacency 1 % dense, symmetric)
  small     2048 graphs of 20-60 nodes, K = 20, F = 32, sparse inputs (edge_index + batch), inference
  train_c2  the c2 inputs, one training step: forward, backward of mean(x_pool^2) + the auxiliary losses

Prints one JSON line.  DMoN is not in pooler_map yet: it is built from its class; MinCut from get_pooler("mincut").
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sync():
    import torch
    ev = torch.cuda.Event()
    ev.record()
    while not ev.query():
        pass
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pooler", choices=("dmon", "mincut"), required=True)
    ap.add_argument("--workload", choices=("c2", "small", "train_c2"), default="c2")
    ap.add_argument("--tree", default=ROOT, help="checkout whose tgp package is imported")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "torch-geometric-pool_amd"))
    import torch
    import tgp
    from tgp.poolers import get_pooler

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    if a.workload in ("c2", "train_c2"):
        B, N, K, F = 32, 1024, 128, 64
        adj = (torch.rand(B, N, N, generator=g) < 0.005)
        adj = (adj | adj.transpose(1, 2)).float().to(dev)
        x = torch.randn(B, N, F, generator=g).to(dev)
        kw = dict(x=x, adj=adj)
    else:
        K, F = 20, 32
        sizes = torch.randint(20, 61, (2048,), generator=g).tolist()
        eis, bs, off = [], [], 0
        for gi, n in enumerate(sizes):
            m = torch.triu(torch.rand(n, n, generator=g) < 4.0 / n, 1)
            eis.append((m | m.t()).nonzero().t() + off)
            bs.append(torch.full((n,), gi))
            off += n
        kw = dict(x=torch.randn(off, F, generator=g).to(dev), adj=torch.cat(eis, 1).to(dev), batch=torch.cat(bs).to(dev))
    if a.pooler == "dmon":
        from tgp.poolers import DMoNPooling
        pooler = DMoNPooling(in_channels=F, k=K)
    else:
        pooler = get_pooler("mincut", in_channels=F, k=K)
    pooler = pooler.to(dev)
    train = a.workload == "train_c2"
    pooler.train(train)
    if train:
        kw["x"] = kw["x"].requires_grad_(True)

    def step():
        if not train:
            with torch.no_grad():
                return pooler(**kw)
        out = pooler(**kw)
        (out.x.square().mean() + sum(out.loss.values())).backward()
        kw["x"].grad = None
        for p in pooler.parameters():
            p.grad = None
        return out

    for _ in range(a.warmup):
        step()
    ms = []
    for _ in range(a.windows):
        _sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        _sync()
        ms.append((time.perf_counter() - t0) / a.steps * 1e3)
    print(json.dumps({"pooler": a.pooler, "workload": a.workload, "tree": os.path.abspath(a.tree),
                      "tgp_file": tgp.__file__, "ms_per_step_median": round(statistics.median(ms), 5),
                      "ms_per_step_min": round(min(ms), 5), "ms_per_step_max": round(max(ms), 5),
                      "windows": a.windows, "steps_per_window": a.steps}))


if __name__ == "__main__":
    main()
