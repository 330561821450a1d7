"""The aggregation readout (GlobalReduce on csrc/segment_aggr.hip) against the composed device form a user writes
without it (``index_add_`` / ``scatter_reduce_``, plus ``x[mask]`` for a masked dense batch), in ONE process, as
alternating pairs of timing windows.

    python tools/bench_readout.py                         # every shape, sum / max / multi(sum, mean, max)
    python tools/bench_readout.py --shapes small --pairs 5

Shapes:
  small   2048 graphs of 20-60 nodes, F = 32, a sorted batch vector
  large   ONE graph of N = 1M nodes, F = 128
  dense   a masked dense batch B = 32, N = 1024, F = 64 (graph sizes 512-1024: a prefix mask)
  mid     32 graphs of exactly 256 nodes, F = 64 (not in the default set): the longest batch that is NOT split into row
          chunks, 32 lane groups of 16 lanes on a device with room for thousands

Every window is ``--steps`` calls between two device synchronisations; a pair is one native and one composed window, back
to back, so both see the same state of the box.  Reported per (shape, operation, mode): the median over the pairs of
each side, the ratio composed / native, and for the native forward the bytes the algorithm has to move (x once + the
output + the mask) over the median call time as a fraction of the 8.0 TB/s HBM peak -- a whole-call figure (launch and
host time included), not a kernel time.  Results are checked against each other before they are timed.  One JSON line
per measurement, then a table.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-geometric-pool_amd"))
HBM_PEAK = 8.0e12


def _sync():
    import torch
    torch.cuda.synchronize()


def composed(x, index, groups, ops):
    """PyG's scatter from torch ops on the device, one op after the other."""
    import torch
    outs = []
    for op in ops:
        out = x.new_zeros(groups, x.size(1))
        if op in ("sum", "mean"):
            out.index_add_(0, index, x)
            if op == "mean":
                count = x.new_zeros(groups).index_add_(0, index, x.new_ones(index.numel())).clamp_(min=1)
                out = out / count.view(-1, 1)
        else:
            out.scatter_reduce_(0, index.view(-1, 1).expand_as(x), x, reduce="amax", include_self=False)
        outs.append(out)
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=-1)


def make_shape(name, dev):
    import torch
    g = torch.Generator().manual_seed(0)
    if name == "small":
        sizes = torch.randint(20, 61, (2048,), generator=g)
        batch = torch.arange(2048).repeat_interleave(sizes)
        return dict(x=torch.randn(batch.numel(), 32, generator=g).to(dev), batch=batch.to(dev), groups=2048, mask=None)
    if name == "mid":
        batch = torch.arange(32).repeat_interleave(256)
        return dict(x=torch.randn(batch.numel(), 64, generator=g).to(dev), batch=batch.to(dev), groups=32, mask=None)
    if name == "large":
        n = 1 << 20
        return dict(x=torch.randn(n, 128, generator=g).to(dev), batch=torch.zeros(n, dtype=torch.long, device=dev),
                    groups=1, mask=None)
    B, N, F = 32, 1024, 64
    sizes = torch.randint(512, 1025, (B,), generator=g)
    mask = torch.arange(N).view(1, -1) < sizes.view(-1, 1)
    return dict(x=torch.randn(B, N, F, generator=g).to(dev), batch=None, groups=B, mask=mask.to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["small", "large", "dense"], choices=("small", "large", "dense", "mid"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    import torch
    from tgp.reduce import GlobalReduce

    assert torch.cuda.is_available(), "bench_readout.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda:0")
    variants = {"sum": ("sum",), "max": ("max",), "multi": ("sum", "mean", "max")}
    rows = []
    for shape in a.shapes:
        s = make_shape(shape, dev)
        x, batch, groups, mask = s["x"], s["batch"], s["groups"], s["mask"]
        F = x.size(-1)
        steps = max(10, a.steps // 5) if shape == "large" else a.steps
        dense_index = None if mask is None else torch.arange(groups, device=dev).repeat_interleave(x.size(1))
        for vname, ops in variants.items():
            reducer = GlobalReduce(vname, aggrs=list(ops)) if vname == "multi" else GlobalReduce(vname)

            def native(t):
                return reducer(t, mask=mask) if mask is not None else reducer(t, batch=batch, size=groups)

            def torch_form(t):
                if mask is not None:  # what the reference does: compact the valid rows, then scatter
                    keep = mask.view(-1)
                    return composed(t[mask], dense_index[keep], groups, ops)
                return composed(t, batch, groups, ops)

            with torch.no_grad():
                got, want = native(x), torch_form(x)
            rows_per_group = x.numel() / F / groups
            torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5 * rows_per_group)
            for mode in ("fwd", "fwd+bwd"):
                xt = x.clone().requires_grad_(True) if mode == "fwd+bwd" else x

                def step(fn):
                    if mode == "fwd":
                        with torch.no_grad():
                            return fn(xt)
                    out = fn(xt)
                    out.square().sum().backward()
                    xt.grad = None
                    return out

                for fn in (native, torch_form):
                    for _ in range(a.warmup):
                        step(fn)
                ms = {"native": [], "composed": []}
                for _ in range(a.pairs):
                    for side, fn in (("native", native), ("composed", torch_form)):
                        _sync()
                        t0 = time.perf_counter()
                        for _ in range(steps):
                            step(fn)
                        _sync()
                        ms[side].append((time.perf_counter() - t0) / steps * 1e3)
                med = {k: statistics.median(v) for k, v in ms.items()}
                moved = x.numel() * 4 + groups * len(ops) * F * 4 + (mask.numel() if mask is not None else 0)
                if mask is not None:  # masked rows are not loaded
                    moved = int(mask.sum()) * F * 4 + groups * len(ops) * F * 4 + mask.numel()
                rec = {"shape": shape, "op": vname, "mode": mode, "steps": steps, "pairs": a.pairs,
                       "native_ms": [round(v, 5) for v in ms["native"]], "composed_ms": [round(v, 5) for v in ms["composed"]],
                       "native_ms_median": round(med["native"], 5), "composed_ms_median": round(med["composed"], 5),
                       "composed_over_native": round(med["composed"] / med["native"], 3),
                       "fwd_bytes": moved if mode == "fwd" else None,
                       "fwd_hbm_fraction_of_call": round(moved / (med["native"] * 1e-3) / HBM_PEAK, 4) if mode == "fwd" else None}
                print(json.dumps(rec), flush=True)
                rows.append(rec)
    print(f"\n{'shape':6} {'op':6} {'mode':8} {'native ms':>10} {'composed ms':>12} {'ratio':>7} {'HBM frac (call)':>16}")
    for r in rows:
        frac = "" if r["fwd_hbm_fraction_of_call"] is None else f"{r['fwd_hbm_fraction_of_call']:.3f}"
        print(f"{r['shape']:6} {r['op']:6} {r['mode']:8} {r['native_ms_median']:10.5f} {r['composed_ms_median']:12.5f} "
              f"{r['composed_over_native']:7.2f} {frac:>16}")


if __name__ == "__main__":
    main()
