"""EigenPooling's parts and whole forward: each native number next to the composed device form on the same inputs -- the
reference's shape, a Python loop over graphs (and, in the selector, over clusters) with ``torch.linalg.eigh`` in float64
and a dense ``Theta [n, K H]`` per graph.  Same timing as bench.py (median of the windows after a warm-up, device
synchronised), measured in alternation inside every window round.

    python tools/bench_eigenpool.py --workload small
    python tools/bench_eigenpool.py --workload large --steps 3 --warmup 1

Workloads (k = 8, H = 5, F = 32):
  small  2048 graphs of 20-60 nodes: every cluster and every graph fits the modes kernel
  large  one graph of 4096 nodes, mean degree 8: the graph (the labeller's embedding) and its clusters of ~512 nodes are
         beyond the kernel's group limit, so the selector's eigenproblems take the composed route on both sides
Timed:
  select / composed_select          EigenPoolSelect: the labeller and the modes / the same labeller with its embedding
                                    from torch.linalg.eigh per graph, then the per-graph, per-cluster eigh loop that
                                    writes dense Thetas
  modes / composed_modes            the selector with the labels given: the modes alone / that loop alone
  reduce_connect / composed_...     Reduce + Connect of a cached selection / Theta_b^T X_b and Omega^T A_ext Omega per graph
  lift / composed_lift              Lift of the pooled features
  forward / composed_forward        select + reduce + connect
  train_step / composed_train       forward (cached selection) + backward of sum(x_pool^2)
The selector's slow runs (select, composed_select, both forwards) take ``--select-steps`` steps per window.
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--select-steps", type=int, default=1)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "torch-geometric-pool_amd"))
    import torch
    from tgp import kernels
    from tgp.poolers import EigenPooling, eigenpool
    from tgp.select import SelectOutput, eigenpool_theta
    from tgp.utils.ops import postprocess_adj_pool_dense

    if not torch.cuda.is_available():
        raise SystemExit("bench_eigenpool.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    k, H, F = 8, 5, 32
    sizes = torch.randint(20, 61, (2048,), generator=g).tolist() if a.workload == "small" else [4096]
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
    ei, ew = torch.cat(eis, 1).to(dev), torch.cat(ews).to(dev)
    batch = torch.cat(bs).to(dev) if len(sizes) > 1 else None
    x = torch.randn(n, F, generator=g).to(dev)
    pool = EigenPooling(k=k, num_modes=H)
    cached = EigenPooling(k=k, num_modes=H)
    with torch.no_grad():
        so = pool.select(edge_index=ei, edge_weight=ew, batch=batch)
    labels = so.s.argmax(-1)
    width = so.s.size(1)
    ptr = [0]
    for s in sizes:
        ptr.append(ptr[-1] + s)
    row_graph = (batch if batch is not None else torch.zeros(n, dtype=torch.long, device=dev))[ei[0]]
    eptr = torch.zeros(len(sizes) + 1, dtype=torch.long)
    eptr[1:] = torch.bincount(row_graph.cpu(), minlength=len(sizes)).cumsum(0)
    eptr = eptr.tolist()  # (the list is grouped by graph)

    def dense_graph(b):
        lo, m = ptr[b], sizes[b]
        e = slice(eptr[b], eptr[b + 1])
        return torch.zeros(m, m, device=dev).index_put_((ei[0, e] - lo, ei[1, e] - lo), ew[e], accumulate=True)

    def composed_labels():
        memo = kernels._adj_symmetric_memo
        kernels._adj_symmetric_memo = lambda *args: False  # "known asymmetric": every eigenproblem takes the composed route
        try:
            gb = batch if batch is not None else torch.zeros(n, dtype=torch.long, device=dev)
            sz = torch.tensor(sizes, device=dev)
            nptr = torch.tensor(ptr, device=dev)
            return eigenpool._spectral_labels(ei, ew, None, gb, sz, nptr, k)
        finally:
            kernels._adj_symmetric_memo = memo

    def composed_select(cluster=True):
        if cluster:
            composed_labels()
        thetas = []
        for b in range(len(sizes)):
            adj = dense_graph(b).double()
            lab = labels[ptr[b]:ptr[b + 1]]
            theta = torch.zeros(sizes[b], width * H, dtype=torch.float64, device=dev)
            for c in range(width):
                nodes = (lab == c).nonzero().view(-1)
                m = nodes.numel()
                if m == 0:
                    continue
                sub = adj[nodes][:, nodes]
                if m == 1:
                    theta[nodes[0], c::width] = sub[0, 0]
                    continue
                dis = 1.0 / torch.sqrt(sub.sum(0) + 1.401298464324817e-45)
                lap = torch.eye(m, dtype=torch.float64, device=dev) - dis.view(-1, 1) * sub * dis.view(1, -1)
                u = torch.linalg.eigh(lap)[1]
                v = u[:, [min(h, m - 1) for h in range(H)]]
                v = torch.where(v[0:1] < 0, -v, v)
                theta[nodes.view(-1, 1), (torch.arange(H, device=dev) * width + c).view(1, -1)] = v
            thetas.append(theta.float())
        return SelectOutput(s=so.s, batch=batch, theta=thetas if batch is not None else thetas[0])

    so_dense = SelectOutput(s=so.s, batch=batch, theta=eigenpool_theta(so))

    def composed_connect():
        out = []
        for b in range(len(sizes)):
            adj = dense_graph(b)
            lab = labels[ptr[b]:ptr[b + 1]]
            omega = so.s[ptr[b]:ptr[b + 1]]
            out.append(omega.t() @ (adj * (lab.view(-1, 1) != lab.view(1, -1))) @ omega)
        return postprocess_adj_pool_dense(torch.stack(out), True, True, False, False)

    def reduce_connect(sel):
        xp = pool.reducer(x, sel, batch=batch)[0]
        return xp, (pool.connector(ei, sel, edge_weight=ew, batch=batch) if sel is so else composed_connect())

    x_pool = reduce_connect(so)[0]

    def train(sel):
        def step():
            xg = x.detach().requires_grad_(True)
            (pool.reducer(xg, sel, batch=batch)[0] ** 2).sum().backward()
            return xg.grad
        return step

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def forward_composed():
        sel = composed_select()
        return pool.reducer(x, sel, batch=batch)[0], composed_connect()

    S = a.select_steps
    runs = {
        "select": (no_grad(lambda: pool.selector(edge_index=ei, edge_weight=ew, batch=batch)), S),
        "modes": (no_grad(lambda: pool.selector(edge_index=ei, edge_weight=ew, batch=batch, labels=labels)), a.steps),
        "composed_select": (no_grad(composed_select), S),
        "composed_modes": (no_grad(lambda: composed_select(False)), S),
        "reduce_connect": (no_grad(lambda: reduce_connect(so)), a.steps),
        "composed_reduce_connect": (no_grad(lambda: reduce_connect(so_dense)), S),
        "lift": (no_grad(lambda: pool.lifter(x_pool, so, batch=batch)), a.steps),
        "composed_lift": (no_grad(lambda: pool.lifter(x_pool, so_dense, batch=batch)), S),
        "forward": (no_grad(lambda: pool(x=x, adj=ei, edge_weight=ew, batch=batch)), S),
        "composed_forward": (no_grad(forward_composed), S),
        "train_step": (train(so), a.steps),
        "composed_train": (train(so_dense), S),
    }
    cached.cached = True
    runs["cached_forward"] = (no_grad(lambda: cached(x=x, adj=ei, edge_weight=ew, batch=batch)), a.steps)
    nat, comp = runs["reduce_connect"][0](), runs["composed_reduce_connect"][0]()
    err = {"x_pool": float((nat[0].double() - comp[0].double()).abs().max()),
           "adj": float((nat[1][0].double() - comp[1].double()).abs().max()),
           "lift": float((runs["lift"][0]().double() - runs["composed_lift"][0]().double()).abs().max()),
           "grad": float((runs["train_step"][0]().double() - runs["composed_train"][0]().double()).abs().max())}
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
    group_sizes = (so.theta_ptr[1:] - so.theta_ptr[:-1])
    out = {"workload": a.workload, "num_graphs": len(sizes), "num_nodes": n, "num_edges": int(ei.size(1)), "k": k,
           "num_modes": H, "features": F, "largest_group": int(group_sizes.max()),
           "group_limit": kernels.eigenpool_max_group_nodes(),
           "modes_route": "composed (over the limit)" if int(group_sizes.max()) > kernels.eigenpool_max_group_nodes()
           else "kernel", "windows": a.windows, "steps_per_window": a.steps, "select_steps_per_window": S,
           "native_vs_composed": err}
    for name in runs:
        out[f"{name}_ms_median"] = round(med[name], 5)
        out[f"{name}_ms_min"] = round(min(ms[name]), 5)
        out[f"{name}_ms_max"] = round(max(ms[name]), 5)
    for part in ("select", "reduce_connect", "lift", "forward"):
        out[f"{part}_over_composed"] = round(med[part] / med[f"composed_{part}"], 5)
    out["modes_over_composed"] = round(med["modes"] / med["composed_modes"], 5)
    out["train_step_over_composed_train"] = round(med["train_step"] / med["composed_train"], 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
