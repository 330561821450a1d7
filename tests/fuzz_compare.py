"""The comparison rule of the seeded family sweep (tests/test_gpu_fuzz_families.py, tests/test_fuzz_inputs.py).

Gradients go through ``grad_path_errors`` of tests/test_gpu_grad_paths.py with its constants.  Forward values go
through :func:`forward_errors`, built on the same principle: for every float output, with r64 the plain-torch
restatement in float64 on the CPU, r32 the same restatement in float32 on the CPU and e(t) = ||t - r64|| / ||r64||,

    e(got) <= bound = max(factor * e(r32), FLOOR),   max|got - r64| <= 4 bound max|r64|,   bound <= CAP.

A bound above CAP means the draw is ill-conditioned for float32: the generator is changed for it, never the cap.
Entries where the float64 reference is not finite (the -inf loss of a graph without a real node) must be equal as they
stand; entries listed in ``zeros`` (padded rows, columns beyond k_b) must be exact zeros.  Integer outputs -- indices,
selections, counts, flags, tie counts -- and float outputs of integer-valued inputs (max / min, exact sums) are handed
in as ``exact`` and compared with ``torch.equal``.

``factor`` is the project's FACTOR unless profiles/fuzz_newer_families.txt states a factor of its own for a family.
"""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_gpu_grad_paths import CAP, F64_BOUND, FACTOR, FLOOR, grad_path_errors  # noqa: E402,F401

# factors that differ from FACTOR, by family, each with its reason in profiles/fuzz_newer_families.txt (none so far)
FAMILY_FACTOR = {}


def factor_of(family):
    return FAMILY_FACTOR.get(family, FACTOR)


def _host64(t):
    return t.detach().to("cpu", torch.float64)


def forward_errors(case, got, ref64, ref32, exact=(), zeros=None, factor=FACTOR, report=None, exact_ref=None):
    """Failure messages (empty: every output is within its bound) of the outputs ``got`` (name -> tensor, any device)
    against ``ref64`` / ``ref32`` (the restatement's outputs by the same names).  ``exact``: names compared with
    ``torch.equal`` (dtype aside) -- with ``exact_ref`` (the float32 restatement: a selection among, or an exact sum of,
    float32 values such as rounded products) instead of ``ref64``.  ``zeros``: name -> bool mask of entries that must be
    exact zeros.  ``report`` (a list) receives (case, output, e_kernel, e_r32) of every float comparison."""
    fails = []
    for name, want in ref64.items():
        where = f"{case}: output {name}"
        if name not in got:
            fails.append(f"{where}: missing from the product")
            continue
        have = got[name]
        if tuple(have.shape) != tuple(want.shape):
            fails.append(f"{where}: shape {tuple(have.shape)} != {tuple(want.shape)}")
            continue
        if name in exact:
            h, w = have.detach().cpu(), (want if exact_ref is None else exact_ref[name]).detach().cpu()
            same = torch.equal(h.to(torch.float64), w.to(torch.float64)) if (h.is_floating_point() or w.is_floating_point()) \
                else torch.equal(h.to(torch.int64), w.to(torch.int64))
            if not same:
                bad = (h.to(torch.float64) != w.to(torch.float64)).nonzero()
                fails.append(f"{where}: not equal to the reference at {bad.size(0)} entries, first {bad[0].tolist()}: "
                             f"{h[tuple(bad[0])].item()} != {w[tuple(bad[0])].item()}")
            continue
        have, want = _host64(have), _host64(want)
        r32 = _host64(ref32[name])
        if zeros is not None and name in zeros:
            z = zeros[name]
            if bool((have[z] != 0).any()):
                fails.append(f"{where}: {int((have[z] != 0).sum())} entries that must be exact zeros are not")
                continue
        fin = torch.isfinite(want)
        if not bool(fin.all()):
            h, w = have[~fin], want[~fin]
            if not bool(((h == w) | (torch.isnan(h) & torch.isnan(w))).all()):
                fails.append(f"{where}: differs where the reference is not finite")
                continue
            have, want, r32 = have[fin], want[fin], r32[fin]
        if want.numel() == 0:
            continue
        if not bool(torch.isfinite(have).all()):
            fails.append(f"{where}: non-finite value where the reference is finite")
            continue
        norm = float(torch.linalg.vector_norm(want))
        if norm == 0:
            if bool((have != 0).any()):
                fails.append(f"{where}: the reference is zero, the product's max |y| = {float(have.abs().max()):.3e}")
            continue
        e_k = float(torch.linalg.vector_norm(have - want)) / norm
        e_32 = float(torch.linalg.vector_norm(r32 - want)) / norm
        bound = max(factor * e_32, FLOOR)
        if report is not None:
            report.append((case, name, e_k, e_32))
        ratio = e_k / e_32 if e_32 > 0 else math.inf
        what = f"{where}: e_kernel {e_k:.3e}, e_r32 {e_32:.3e}, e_kernel/e_r32 {ratio:.3g}, bound {bound:.3e}"
        if bound > CAP:
            fails.append(f"{what}: the bound exceeds {CAP:g} (ill-conditioned data)")
            continue
        if e_k > bound:
            fails.append(f"{what}: normwise error above the bound")
            continue
        worst = float((have - want).abs().max())
        if worst > 4 * bound * float(want.abs().max()):
            fails.append(f"{what}: max |y - r64| = {worst:.3e} above 4 bound max|r64| = "
                         f"{4 * bound * float(want.abs().max()):.3e}")
    return fails


def print_report(report, kind="forward"):
    """One line per comparison, as ``check_grad_paths`` prints them."""
    for case, name, e_k, e_32 in report:
        ratio = e_k / e_32 if e_32 > 0 else float("nan")
        print(f"FUZZ {kind} | {case} | {name} | e_kernel {e_k:.2e} | e_r32 {e_32:.2e} | ratio {ratio:.3g}")


def print_grad_report(case, report):
    for path, leaf, e_k, e_32 in report:
        ratio = e_k / e_32 if e_32 > 0 else float("nan")
        print(f"FUZZ grad | {case} | {path}->{leaf} | e_kernel {e_k:.2e} | e_r32 {e_32:.2e} | ratio {ratio:.3g}")


def conditioning(ref64, ref32):
    """Largest e(r32) over the float outputs: the reference alone must stay within CAP / FACTOR."""
    worst = 0.0
    for name, want in ref64.items():
        if not want.is_floating_point():
            continue
        want, r32 = _host64(want), _host64(ref32[name])
        fin = torch.isfinite(want)
        norm = float(torch.linalg.vector_norm(want[fin]))
        if norm > 0:
            worst = max(worst, float(torch.linalg.vector_norm(r32[fin] - want[fin])) / norm)
    return worst
