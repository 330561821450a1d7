#!/usr/bin/env python3
"""Worst e_kernel / e_r32 per family, layer and output from the ``FUZZ`` lines of
``python -m pytest tests/test_gpu_fuzz_families.py -q -s > LOG``: the body of profiles/fuzz_newer_families.txt.

A comparison whose float32 restatement is exact (e_r32 = 0) has no ratio; it is held to the floor and listed by its
e_kernel.  "binding": the worst ratio among the comparisons whose bound is FACTOR * e_r32 rather than the floor
(FACTOR * e_r32 > FLOOR), and how many those are -- the only ones on which the factor is exercised.
usage: fuzz_ratios.py LOG [FACTOR FLOOR]   (defaults: the constants of tests/test_gpu_grad_paths.py, 16 and 2e-6)"""
import collections
import re
import sys


def main(path, factor=16.0, floor=2e-6):
    worst = collections.OrderedDict()
    for line in open(path):
        at = line.find("FUZZ ")
        if at < 0:
            continue
        f = [t.strip() for t in line[at:].split("|")]
        if len(f) < 6:
            continue
        kind, case, name = f[0].split()[1], f[1], re.sub(r"\[\d+\]", "[*]", f[2])
        e_k, e_32 = float(f[3].split()[1]), float(f[4].split()[1])
        key = (re.sub(r"-\d+.*$", "", case), kind, name)
        w = worst.setdefault(key, {"n": 0, "ratio": 0.0, "case": "", "exact_ek": 0.0, "ek": 0.0, "e32": 0.0, "bind": 0.0,
                                   "nbind": 0})
        w["n"] += 1
        if factor * e_32 > floor:
            w["nbind"] += 1
            w["bind"] = max(w["bind"], e_k / e_32)
        if e_32 > 0:
            if e_k / e_32 >= w["ratio"]:
                w.update(ratio=e_k / e_32, case=case, ek=e_k, e32=e_32)
        else:
            w["exact_ek"] = max(w["exact_ek"], e_k)
    print(f"{'family-layer':<22}{'kind':<9}{'output':<22}{'compared':>9}{'worst ratio':>13}{'e_kernel':>11}{'e_r32':>11}"
          f"{'binding: n':>12}{'worst':>8}{'e_kernel where e_r32 = 0':>27}  worst case")
    for (fam, kind, name), w in worst.items():
        print(f"{fam:<22}{kind:<9}{name:<22}{w['n']:>9}{w['ratio']:>13.3g}{w['ek']:>11.2e}{w['e32']:>11.2e}"
              f"{w['nbind']:>12}{w['bind']:>8.3g}{w['exact_ek']:>27.2e}  {w['case']}")


if __name__ == "__main__":
    main(sys.argv[1], *(float(a) for a in sys.argv[2:4]))
