"""BN-Pool against MinCut, and BN-Pool's reconstruction loss (native: the logits S K S^T are never written) against the
composed form that multiplies them out: the same inputs, the same timing as bench.py (median of 5 windows of steps).

    python tools/bench_bnpool.py --pooler bnpool --workload c2              # this tree, whole forward
    python tools/bench_bnpool.py --pooler mincut --workload c2 --tree DIR   # another checkout (e.g. the parent commit)
    python tools/bench_bnpool.py --pooler bnpool   --workload loss_c2       # the reconstruction loss alone, native
    python tools/bench_bnpool.py --pooler composed --workload loss_c2       # the same loss as fp32 torch ops on the device
    ... --backward                                                          # forward + backward to S and K

Workloads:
  c2          dense padded inference, B = 32 graphs x N = 1024 nodes, K = 128, F = 64 (adjacency 1 % dense)
  loss_c2     the reconstruction loss alone on the c2 adjacency, S = stick-breaking of seeded sticks, asymmetric K
  loss_small  the same on 2048 graphs of 20-60 nodes densified to [2048,60,60] with their mask, K = 20

Prints one JSON line: the median time, the peak of allocated memory one step adds, and for the loss workloads the rate
of the logit product (2 B N^2 K flop per product: one in the forward; the native backward forms four more, two logit
recomputations and the two products with G).  BN-Pool is not in pooler_map yet: it is built from its class.
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


def _small_adjacency(torch, g, dev):
    sizes = torch.randint(20, 61, (2048,), generator=g)
    n = int(sizes.max())
    adj = torch.zeros(2048, n, n)
    for gi, m in enumerate(sizes.tolist()):
        a = torch.triu(torch.rand(m, m, generator=g) < 4.0 / m, 1)
        adj[gi, :m, :m] = (a | a.t()).float()
    mask = torch.arange(n).unsqueeze(0) < sizes.unsqueeze(1)
    return adj.to(dev), mask.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pooler", choices=("bnpool", "mincut", "composed"), required=True)
    ap.add_argument("--workload", choices=("c2", "loss_c2", "loss_small"), default="c2")
    ap.add_argument("--backward", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="checkout whose tgp package is imported")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "torch-geometric-pool_amd"))
    import torch
    import tgp
    from tgp.poolers import get_pooler

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    flop = None
    if a.workload == "c2":
        B, N, K, F = 32, 1024, 128, 64
        adj = (torch.rand(B, N, N, generator=g) < 0.005)
        adj = (adj | adj.transpose(1, 2)).float().to(dev)
        x = torch.randn(B, N, F, generator=g).to(dev)
        if a.pooler == "mincut":
            pooler = get_pooler("mincut", in_channels=F, k=K).to(dev).eval()
        elif a.pooler == "bnpool":
            from tgp.poolers import BNPool
            pooler = BNPool(in_channels=F, k=K).to(dev).eval()
        else:
            raise SystemExit("the whole forward compares --pooler bnpool with --pooler mincut")

        def step():
            with torch.no_grad():
                return pooler(x=x, adj=adj)
    else:
        if a.pooler == "mincut":
            raise SystemExit("the loss workloads compare --pooler bnpool (native) with --pooler composed")
        from tgp.utils.losses import bnpool_rec_loss_terms, weighted_bce_reconstruction_loss
        if a.workload == "loss_c2":
            B, N, K = 32, 1024, 128
            adj = (torch.rand(B, N, N, generator=g) < 0.005)
            adj = (adj | adj.transpose(1, 2)).float().to(dev)
            mask = torch.ones(B, N, dtype=torch.bool, device=dev)
        else:
            K = 20
            adj, mask = _small_adjacency(torch, g, dev)
            B, N = adj.shape[:2]
        z = torch.rand(B, N, K - 1, generator=g).to(dev) * 0.5 + 0.05
        pad = z.new_zeros(B, N, 1)
        S = torch.exp(torch.cat([z.log(), pad], -1) + torch.cat([pad, (1 - z).log().cumsum(-1)], -1)) * mask.unsqueeze(-1)
        Km = torch.randn(K, K, generator=g).to(dev)
        n2 = mask.sum(-1) ** 2
        flop = 2.0 * B * N * N * K
        if a.backward:
            S.requires_grad_(True)
            Km.requires_grad_(True)

        def loss():
            if a.pooler == "bnpool":
                return bnpool_rec_loss_terms(S, Km, adj, mask).mean()
            return weighted_bce_reconstruction_loss(S @ Km @ S.transpose(-1, -2), adj, mask, normalizing_const=n2)

        def step():
            if not a.backward:
                with torch.no_grad():
                    return loss()
            out = loss()
            out.backward()
            S.grad = Km.grad = None
            return out

    for _ in range(a.warmup):
        step()
    _sync()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    _sync()
    peak = torch.cuda.max_memory_allocated() - base
    ms = []
    for _ in range(a.windows):
        _sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        _sync()
        ms.append((time.perf_counter() - t0) / a.steps * 1e3)
    med = statistics.median(ms)
    out = {"pooler": a.pooler, "workload": a.workload, "backward": a.backward, "tree": os.path.abspath(a.tree),
           "tgp_file": tgp.__file__, "ms_per_step_median": round(med, 5), "ms_per_step_min": round(min(ms), 5),
           "ms_per_step_max": round(max(ms), 5), "windows": a.windows, "steps_per_window": a.steps,
           "peak_bytes_per_step": int(peak)}
    if flop is not None:
        products = 5 if (a.backward and a.pooler == "bnpool") else 3 if a.backward else 1
        out["logit_product_flop"] = flop
        out["products_per_step"] = products
        out["tflops_of_the_products"] = round(products * flop / (med * 1e-3) / 1e12, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
