"""A two-level model (MinCut -> relu(A' X' W) -> DiffPool -> readout): the second pooler is handed the first one's pooled
adjacency, a dense [B,K1,K1] activation that requires a gradient.  With the native adjacency gradient
(csrc/dense_adj_grad.hip; tgp.poolers._ADJ_GRAD) the second level stays on the one-node training routes; with the flag
off it takes the operator route, which is what the commit before did for these calls.

    python tools/bench_stacked.py                       # both shapes and the kernel alone
    python tools/bench_stacked.py --only c2 --steps 50

Shapes:
  c2     32 graphs x 1024 nodes (adjacency 1 % dense), K1 = 128, K2 = 32, F = 64
  small  2048 graphs of 20-60 nodes padded to 60 (mask), K1 = 20, K2 = 5, F = 32
  kernel the new tiled kernel alone at S [32,1024,128] and [32,128,32] (T = S M, then T S^T + gamma q + c A in one
         launch) next to torch.bmm(S, M), torch.bmm(T, S^T) and the two elementwise adds, with its share of the HBM
         (8 TB/s; A read once + dA written once) and fp32-matrix (157.3 TFLOP/s; 2 B N^2 K) rooflines

Timing as bench.py: windows of --steps steps, each closed by a device synchronise; the flag-on and flag-off windows
ALTERNATE in one process on one box (on, off, on, off, ...) and the medians of the windows are reported with their range.
Launches per step and GPU-busy time come from one profiled step (torch.profiler).  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-geometric-pool_amd"))

HBM_BYTES_PER_S = 8.0e12
FP32_MATRIX_FLOPS = 157.3e12


def _sync():
    import torch
    torch.cuda.synchronize()


def _window(step, steps):
    _sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    _sync()
    return (time.perf_counter() - t0) / steps * 1e3


def _spread(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5)}


def _profile(step):
    import torch
    from torch.profiler import ProfilerActivity, profile
    step()
    _sync()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        _sync()
    evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(evs), round(sum(e.device_time for e in evs) / 1e3, 4)


def _alternate(make_step, a):
    """{flag: spread} of make_step(flag)'s windows, flag on and off alternating."""
    import tgp.poolers as P
    steps = {}
    for flag in (True, False):
        P._ADJ_GRAD = flag
        steps[flag] = make_step()
        for _ in range(a.warmup):
            steps[flag]()
    ms = {True: [], False: []}
    for _ in range(a.windows):
        for flag in (True, False):
            P._ADJ_GRAD = flag
            ms[flag].append(_window(steps[flag], a.steps))
    out = {}
    for flag in (True, False):
        P._ADJ_GRAD = flag
        launches, busy = _profile(steps[flag])
        out["adj_grad_on" if flag else "adj_grad_off"] = dict(_spread(ms[flag]), launches_per_step=launches, gpu_busy_ms=busy)
    P._ADJ_GRAD = True
    return out


def _model(shape, a):
    import torch
    from tgp.poolers import _DenseMLPPooling, get_pooler
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    if shape == "c2":
        B, N, K1, K2, F = 32, 1024, 128, 32, 64
        adj = torch.rand(B, N, N, generator=g) < 0.005
        adj = (adj | adj.transpose(1, 2)).float().to(dev)
        mask = None
    else:
        B, N, K1, K2, F = 2048, 60, 20, 5, 32
        sizes = torch.randint(20, 61, (B, 1), generator=g)
        mask = torch.arange(N).unsqueeze(0) < sizes
        adj = torch.rand(B, N, N, generator=g) < 4.0 / sizes.unsqueeze(-1)
        adj = (adj | adj.transpose(1, 2)) & mask.unsqueeze(1) & mask.unsqueeze(2)
        adj, mask = adj.float().to(dev), mask.to(dev)
    x = torch.randn(B, N, F, generator=g).to(dev)
    if mask is not None:
        x = x * mask.unsqueeze(-1)
    pool1 = get_pooler("mincut", in_channels=F, k=K1).to(dev).train()
    lin = torch.nn.Linear(F, F, bias=False).to(dev)
    pool2 = get_pooler("diff", in_channels=F, k=K2).to(dev).train()
    params = list(pool1.parameters()) + list(lin.parameters()) + list(pool2.parameters())
    routes = []

    def spy(name):
        orig = getattr(_DenseMLPPooling, name)

        def wrapper(this, *args, **kw):
            r = orig(this, *args, **kw)
            if r is not None and this is pool2:
                routes.append(name)
            return r
        return wrapper

    def forward():
        o1 = pool1(x=x, adj=adj, mask=mask)
        hid = torch.relu(o1.edge_index @ lin(o1.x))
        o2 = pool2(x=hid, adj=o1.edge_index)
        return o2.x.mean(dim=1).square().mean() + sum(o1.loss.values()) + sum(o2.loss.values())

    def train():
        forward().backward()
        for p in params:
            p.grad = None

    # which route the second level takes, flag on and off (the spies are removed before anything is timed)
    import tgp.poolers as P
    names = ("_select_reduce_connect_train", "_select_reduce_connect_large")
    saved = {n: getattr(_DenseMLPPooling, n) for n in names}
    second = {}
    for flag in (True, False):
        P._ADJ_GRAD = flag
        for n in names:
            setattr(_DenseMLPPooling, n, spy(n))
        del routes[:]
        forward()
        second["on" if flag else "off"] = routes[0] if routes else None
        for n in names:
            setattr(_DenseMLPPooling, n, saved[n])
    P._ADJ_GRAD = True
    row = {"shape": shape, "B": B, "N": N, "K1": K1, "K2": K2, "F": F, "second_level_route": second}
    row["forward"] = _alternate(lambda: forward, a)
    row["train_step"] = _alternate(lambda: train, a)
    return row


def _kernel(B, N, K, a):
    import torch
    from tgp import kernels as Kn
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    s = torch.softmax(torch.randn(B, N, K, generator=g), -1).to(dev)
    adj = (torch.rand(B, N, N, generator=g) < 0.01).float().to(dev)
    m = torch.randn(B, K, K, generator=g).to(dev)
    gamma = torch.randn(B, generator=g).to(dev)
    q = (s * s).sum(-1)
    g_link, link_loss = torch.tensor(0.7, device=dev), torch.tensor(3.0, device=dev)
    c = 0.7 / 3.0

    def native():
        return Kn.dense_pool_adj_grad(s, adj, m, gamma=gamma, q=q, g_link=g_link, link_loss=link_loss, link_scale=1.0)

    def composed():
        out = torch.bmm(torch.bmm(s, m), s.transpose(1, 2))
        out += (gamma.view(-1, 1) * q).unsqueeze(-1)
        out += c * adj
        return out

    err = float((native() - composed()).abs().max() / composed().abs().max())
    for fn in (native, composed):
        for _ in range(a.warmup):
            fn()
    ms = {"native": [], "composed": []}
    for _ in range(a.windows):  # (alternating)
        ms["native"].append(_window(native, a.steps))
        ms["composed"].append(_window(composed, a.steps))
    row = {"kernel": "dense_pool_adj_grad", "S": [B, N, K], "max_rel_diff_native_vs_composed": err}
    for k, fn in (("native", native), ("composed", composed)):
        launches, busy = _profile(fn)
        row[k] = dict(_spread(ms[k]), launches=launches, gpu_busy_ms=busy)
    t = row["native"]["gpu_busy_ms"] * 1e-3
    row["native"]["hbm_share"] = round(2.0 * B * N * N * 4 / t / HBM_BYTES_PER_S, 4)
    row["native"]["fp32_matrix_share"] = round(2.0 * B * N * N * K / t / FP32_MATRIX_FLOPS, 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("c2", "small", "kernel"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    for shape in ("c2", "small"):
        if a.only in (None, shape):
            print(json.dumps(dict(_model(shape, a), windows=a.windows, steps_per_window=a.steps)), flush=True)
    if a.only in (None, "kernel"):
        for B, N, K in ((32, 1024, 128), (32, 128, 32)):
            print(json.dumps(dict(_kernel(B, N, K, a), windows=a.windows, steps_per_window=a.steps)), flush=True)


if __name__ == "__main__":
    main()
