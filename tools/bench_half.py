"""bf16 rows through the 16-bit storage kernels (csrc/sparse_half.hip) against the upcast route of the same commit,
``op(x.float()).to(x.dtype)``, on one device in alternating windows: the sparse Reduce, the one-to-one Reduce, the Lift
and the readout (sum and multi(sum, mean, max)).

    python tools/bench_half.py [--windows 9] [--out profiles/half_forward.txt]

Per line: the median window of each route (microseconds per call), each route's window spread (max - min over the
median), the ratio, and the new route's effective TB/s from the bytes it has to move (16-bit rows in, 16-bit rows out,
the index tables).  A route wins only by more than the spreads."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-geometric-pool_amd"))

from tgp import kernels as K  # noqa: E402
from tgp.lift import BaseLift  # noqa: E402
from tgp.reduce import BaseReduce, GlobalReduce  # noqa: E402
from tgp.select import SelectOutput  # noqa: E402

DEV = torch.device("cuda:0")


def window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def compare(name, new, upcast, nbytes, windows, lines):
    assert torch.equal(new().view(torch.int16), upcast().view(torch.int16)), name  # faster and different is not faster
    for fn in (new, upcast):
        window(fn, 5)
    iters = max(5, min(200, int(2e4 / max(window(upcast, 5), 1.0))))  # ~20 ms of work per window
    t = {"new": [], "upcast": []}
    for _ in range(windows):
        t["new"].append(window(new, iters))
        t["upcast"].append(window(upcast, iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
    line = (f"{name:<44} new {med['new']:9.1f} us (spread {spread['new']:.3f})  upcast {med['upcast']:9.1f} us "
            f"(spread {spread['upcast']:.3f})  upcast/new {med['upcast'] / med['new']:5.2f}x  "
            f"new route {nbytes / med['new'] / 1e6:5.2f} TB/s")
    print(line, flush=True)
    lines.append(line)


def assignment(node, cluster, n, k, one_to_one):
    w = torch.rand(node.numel(), device=DEV) + 0.5
    so = SelectOutput(cluster_index=cluster, node_index=node, weight=w, num_nodes=n, num_supernodes=k, _trusted=True)
    if one_to_one:
        so._assign_index = K.one_to_one_index(so.node_index, so.cluster_index, so.weight)
    return so


def shape(tag, batch, F, windows, lines):
    """Every operator on one un-padded batch: pairs of neighbours as supernodes, every second node kept, per-graph readout."""
    n, G = batch.numel(), int(batch.max()) + 1
    x = torch.randn(n, F, device=DEV).bfloat16()
    up = lambda fn, t: (lambda: fn(t.float()).to(t.dtype))
    pairs = assignment(torch.arange(n, device=DEV), torch.arange(n, device=DEV) // 2, n, (n + 1) // 2, False)
    kept = torch.arange(0, n, 2, device=DEV)
    k = kept.numel()
    topk = assignment(kept, torch.randperm(k, device=DEV), n, k, True)
    xp = torch.randn(k, F, device=DEV).bfloat16()
    index = 16 * n  # node id 8, weight 4, table entry 4 bytes per assignment
    ops = [("sparse Reduce (2 members)", lambda t: BaseReduce()(t, pairs)[0], x, 2 * n * F + n * F + index + 2 * n),
           ("one-to-one Reduce (every 2nd node)", lambda t: BaseReduce()(t, topk)[0], x, 2 * k * F * 2 + 8 * k),
           ("Lift of it", lambda t: BaseLift(matrix_op="transpose")(t, topk), xp, 2 * k * F + 2 * n * F + 16 * k + 4 * n),
           ("readout sum", lambda t: GlobalReduce("sum")(t, batch=batch, size=G), x, 2 * n * F + 2 * G * F),
           ("readout multi(sum, mean, max)", lambda t: GlobalReduce("multi", aggrs=["sum", "mean", "max"])(t, batch=batch, size=G),
            x, 2 * n * F + 6 * G * F)]
    for name, fn, t, nbytes in ops:
        compare(f"{tag}: {name}", lambda: fn(t), up(fn, t), nbytes, windows, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_half needs the GPU"
    torch.manual_seed(0)
    lines = ["# bf16 rows: 16-bit storage kernels (new) against op(x.float()).to(bf16) (upcast), alternating windows, "
             f"{args.windows} per route, on {torch.cuda.get_device_name(0)}"]
    shape("N=1M F=128, 1024 graphs", torch.arange(1 << 20, device=DEV) // 1024, 128, args.windows, lines)
    sizes = torch.randint(20, 61, (2048,), generator=torch.Generator().manual_seed(0))
    shape("2048 graphs of 20-60 nodes, F=32", torch.repeat_interleave(torch.arange(2048), sizes).to(DEV), 32, args.windows, lines)
    B, Nn, F = 32, 1024, 64
    xd = torch.randn(B, Nn, F, device=DEV).bfloat16()
    mask = torch.arange(Nn, device=DEV).view(1, -1) < torch.randint(Nn // 2, Nn + 1, (B, 1), device=DEV)
    moved = 2 * int(mask.sum()) * F + B * Nn
    for name, op, cols in (("readout sum", GlobalReduce("sum"), 1),
                           ("readout multi(sum, mean, max)", GlobalReduce("multi", aggrs=["sum", "mean", "max"]), 3)):
        compare(f"masked dense 32 x 1024, F=64: {name}", lambda: op(xd, mask=mask), lambda: op(xd.float(), mask=mask).to(xd.dtype),
                moved + 2 * cols * B * F, args.windows, lines)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
