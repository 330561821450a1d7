"""tgp_dense_pool_f32 at the C2 shape (32 graphs, N = 1024, K = 128, F = 64) across the density of A: the dense/sparse
chunk threshold of the first product (gemm_mfma.h, TGP_SPARSE_CHUNK_GROUPS) is set from this sweep.

  python tools/c2_density_sweep.py                     this process's library (TGP_HIP_LIB or the package's)
  python tools/c2_density_sweep.py --ab libA libB ...  the libraries alternated in child processes, two rounds each
  --shape B N K F                                      another batch shape (default C2: 32 1024 128 64)

Two timings per density, median of 5 windows of 50 calls: `same` re-reads one A (134 MB: resident in the 256 MiB
Infinity Cache, as in bench.py's loop), `fresh` rotates three distinct A tensors (402 MB together), so every call
reads its A from HBM.  `GB/s` = bytes of A per call / time (the first product's floor)."""
import argparse
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DENSITIES = [0.001, 0.005, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 1.0]
B, N, KC, F = 32, 1024, 128, 64


def _time(fn, calls=50, windows=5):
    for _ in range(10):
        fn(0)
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / calls)
    return sorted(ts)[windows // 2]


def sweep(densities, shape):
    B, N, KC, F = shape
    sys.path.insert(0, os.path.join(HERE, "..", "torch-geometric-pool_amd"))
    from tgp import kernels as K
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    S = torch.softmax(torch.randn(B, N, KC, device=dev, generator=g), -1)
    X = torch.randn(B, N, F, device=dev, generator=g)
    flags = K.dense_flags(True, True, True, False)
    rows = []
    for p in densities:
        As = []
        for _ in range(3 if B * N * N * 4 * 3 < (8 << 30) else 1):
            a = (torch.rand(B, N, N, device=dev, generator=g) < p / 2).float()  # symmetrised below: density ~p
            a = torch.maximum(a, a.transpose(1, 2)).contiguous()
            a.diagonal(dim1=1, dim2=2).zero_()
            As.append(a)
        same = _time(lambda i: K.dense_pool(S, As[0], X, flags))
        fresh = _time(lambda i: K.dense_pool(S, As[i % len(As)], X, flags))
        nbytes = As[0].numel() * 4
        rows.append({"p": p, "density": round(float((As[0] != 0).float().mean()), 5), "same_us": round(same * 1e3, 2),
                     "fresh_us": round(fresh * 1e3, 2), "fresh_GBps_of_A": round(nbytes / (fresh * 1e-3) / 1e9, 1)})
        del As
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", nargs="+", help="libraries to alternate (child processes, TGP_HIP_LIB)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--densities", type=float, nargs="+", default=DENSITIES)
    ap.add_argument("--shape", type=int, nargs=4, default=[B, N, KC, F], metavar=("B", "N", "K", "F"))
    ap.add_argument("--json", action="store_true", help="(child) print the rows as one JSON line")
    args = ap.parse_args()
    if not args.ab:
        rows = sweep(args.densities, args.shape)
        if args.json:
            print(json.dumps(rows))
        else:
            for r in rows:
                print(r)
        return
    res = {lib: [] for lib in args.ab}
    for _ in range(args.rounds):
        for lib in args.ab:
            env = dict(os.environ, TGP_HIP_LIB=os.path.abspath(lib))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--json", "--densities",
                                  *map(str, args.densities), "--shape", *map(str, args.shape)], env=env, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                sys.exit(f"{lib}: exit {out.returncode}\n{out.stderr[-2000:]}")
            res[lib].append(json.loads(out.stdout.strip().splitlines()[-1]))
    names = [os.path.basename(lib) for lib in args.ab]
    print("p      density  " + "  ".join(f"{n + ' same/fresh us (min..max)':>44}" for n in names))
    for i, p in enumerate(args.densities):
        cells = []
        for lib in args.ab:
            s = [r[i]["same_us"] for r in res[lib]]
            f = [r[i]["fresh_us"] for r in res[lib]]
            cells.append(f"{min(s):7.2f}..{max(s):7.2f} / {min(f):7.2f}..{max(f):7.2f}")
        print(f"{p:<6} {res[args.ab[0]][0][i]['density']:<8} " + "  ".join(f"{c:>44}" for c in cells))
    print(json.dumps({os.path.basename(k): v for k, v in res.items()}))


if __name__ == "__main__":
    main()
