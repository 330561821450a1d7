"""ASAPooling's fitness (attention + LEConv score) and whole forward: the native kernels against the composed device
form, next to TopkPooling's and SAGPooling's forwards on the same inputs and the forward + backward step; the same
timing as bench.py (median of 5 windows after a warm-up, device synchronised), all measured in alternation inside every
window round.

    python tools/bench_asap.py --workload small
    python tools/bench_asap.py --workload large --steps 10 --warmup 3
    python tools/bench_asap.py --workload hub --steps 10 --warmup 3

Workloads:
  small  2048 graphs of 20-60 nodes, F = 32
  large  one graph, N = 1M, E = 10M entries, F = 128
  hub    one graph, N = 65536, 524288 random edges and ONE node of in-degree 524288, F = 128: one wave walks the hub
Timed (every list already carries its self-loops; the augmented list and its by-destination index are remembered):
  native_fitness   ASAPooling.fitness: project, master query, edge softmax, attend (+ projections), LEConv aggregate
  project / query / softmax / attend / leconv   each kernel alone on the same operands
  composed_fitness the same function as ATen ops on the device (three E' x F gathers, scatter-max, two scatter-adds)
  forward          the whole ASAPooling forward (inference)
  topk_forward, sag_forward   TopkPooling's and SAGPooling's forwards on the same batch
  train_step       ASAPooling forward + backward of sum(x_pool^2): the two native autograd nodes
  composed_train   the fitness as ATen ops under autograd, forward + backward of sum((x_new s)^2)
  native_train     the same objective through the native nodes
Bytes counted per kernel (gathered rows are counted once per edge: they are the traffic of a gather kernel, from L2 or
HBM; ``idx`` = 8 E' source ids + 4 E' positions on the permutation route + 4 N offsets):
  query    idx + 4 E' F gathered + 4 N written          softmax  3 idx (three passes) + 4 E' written
  attend   idx + 4 E' alpha + 4 E' F gathered + 4 N F + 12 N written       leconv   idx + 12 N read + 4 N written
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("small", "large", "hub"), default="small")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "torch-geometric-pool_amd"))
    import torch
    from tgp import kernels
    from tgp.poolers import ASAPooling, SAGPooling, TopkPooling
    from tgp.utils import add_remaining_self_loops

    if not torch.cuda.is_available():
        raise SystemExit("bench_asap.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
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
    asap = ASAPooling(in_channels=F).to(dev).eval()
    sag = SAGPooling(in_channels=F).to(dev).eval()
    topk = TopkPooling(in_channels=F).to(dev).eval()
    ea, _ = add_remaining_self_loops(ei, None, num_nodes=n)
    E = int(ea.size(1))
    grp = kernels.sag_edge_group(ea, n)
    le = asap.select_scorer
    with torch.no_grad():
        att = asap.att.weight.view(-1)
        w_tilde = att[:F] @ asap.lin.weight
        c = (att[:F] @ asap.lin.bias + asap.att.bias.view(())).view(1)
        a2 = att[F:].contiguous()
        w3 = le.projections()
        sp, _ = kernels.row_project2(x, a2, a2)
        sq = kernels.asap_query(grp, ea[0], x, w_tilde, c)
        alpha = kernels.asap_edge_softmax(grp, ea[0], sq, sp, 0.2)
        _, p3 = kernels.asap_attend(grp, ea[0], x, alpha, w3)

    def native_fitness():
        with torch.no_grad():
            return asap.fitness(x, ea, None, act="sigmoid")

    def composed_fitness():
        with torch.no_grad():
            al, x_new = asap.attention(x, x, ea)
            msg = le.lin1(x_new)[ea[0]] - le.lin2(x_new)[ea[1]]
            return al, x_new, torch.sigmoid(msg.new_zeros(n, 1).index_add_(0, ea[1], msg) + le.lin3(x_new)).view(-1)

    def forward():
        with torch.no_grad():
            return asap(x=x, adj=ei, batch=batch)

    def train_step():
        asap.zero_grad(set_to_none=True)
        out = asap(x=x, adj=ei, batch=batch)
        (out.x ** 2).sum().backward()

    def _objective(route):
        asap.zero_grad(set_to_none=True)
        xg = x.detach().requires_grad_(True)
        if route == "native":
            _, x_new, s_ = asap.fitness(xg, ea, None, act="sigmoid")
        else:
            _, x_new = asap.attention(xg, xg, ea)
            msg = le.lin1(x_new)[ea[0]] - le.lin2(x_new)[ea[1]]
            s_ = torch.sigmoid(msg.new_zeros(n, 1).index_add_(0, ea[1], msg) + le.lin3(x_new)).view(-1)
        ((x_new * s_.view(-1, 1)) ** 2).sum().backward()

    asap.train()  # dropout = 0: the routes are those of eval, with gradients
    runs = {
        "native_fitness": native_fitness,
        "native_train": lambda: _objective("native"),
        "composed_train": lambda: _objective("composed"),
        "project": lambda: kernels.row_project2(x, a2, a2),
        "query": lambda: kernels.asap_query(grp, ea[0], x, w_tilde, c),
        "softmax": lambda: kernels.asap_edge_softmax(grp, ea[0], sq, sp, 0.2),
        "attend": lambda: kernels.asap_attend(grp, ea[0], x, alpha, w3),
        "leconv": lambda: kernels.asap_leconv(grp, ea[0], p3, None, le.lin1.bias.detach(), le.lin3.bias.detach(), "sigmoid"),
        "composed_fitness": composed_fitness,
        "forward": forward,
        "topk_forward": lambda: _no_grad(torch, topk, x, ei, batch),
        "sag_forward": lambda: _no_grad(torch, sag, x, ei, batch),
        "train_step": train_step,
    }
    nat, comp = native_fitness(), composed_fitness()
    err = {k: float((u.double() - v.double()).abs().max()) for k, u, v in zip(("alpha", "x_new", "score"), nat, comp)}
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
    out = {"workload": a.workload, "num_nodes": n, "num_edges": int(ei.size(1)), "num_edges_with_loops": E,
           "features": F, "index_route": "offsets" if grp.perm is None else "permutation",
           "max_in_degree": int((grp.row_ptr[1:] - grp.row_ptr[:-1]).max()),
           "supernodes": int(forward().so.num_supernodes), "windows": a.windows, "steps_per_window": a.steps,
           "native_vs_composed_max_abs_diff": err}
    for name in runs:
        out[f"{name}_ms_median"] = round(med[name], 5)
        out[f"{name}_ms_min"] = round(min(ms[name]), 5)
        out[f"{name}_ms_max"] = round(max(ms[name]), 5)
    out["native_fitness_over_composed"] = round(med["native_fitness"] / med["composed_fitness"], 4)
    out["native_train_over_composed"] = round(med["native_train"] / med["composed_train"], 4)
    out["forward_over_sag_forward"] = round(med["forward"] / med["sag_forward"], 4)
    out["forward_over_topk_forward"] = round(med["forward"] / med["topk_forward"], 4)
    idx = 8 * E + (4 * E if grp.perm is not None else 0) + 4 * n
    counted = {"project": 4 * n * F + 8 * n, "query": idx + 4 * E * F + 4 * n, "softmax": 3 * idx + 4 * E,
               "attend": idx + 4 * E + 4 * E * F + 4 * n * F + 12 * n, "leconv": idx + 16 * n}
    for name, b in counted.items():
        out[f"{name}_bytes_counted"] = b
        out[f"{name}_share_of_hbm_peak"] = round(b / (med[name] * 1e-3) / HBM_PEAK, 4)
    print(json.dumps(out))


def _no_grad(torch, pooler, x, ei, batch):
    with torch.no_grad():
        return pooler(x=x, adj=ei, batch=batch)


if __name__ == "__main__":
    main()
