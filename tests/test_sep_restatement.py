"""The brute-force restatement of the SEP selector (tests/sep_restatement.py) against the reference's stored results
(tests/golden/golden_sep_v1.pt), its two arithmetic modes against each other, and its equivariance under relabelling."""
import os

import numpy as np
import pytest
import torch

import sep_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_sep_v1.pt"), weights_only=True)["cases"]


def run(c, arith, gaps=None):
    i = c["inputs"]
    return R.sep_select(i["x"].size(0), i["edge_index"].numpy(),
                        None if i["edge_weight"] is None else i["edge_weight"].numpy(),
                        None if i["batch"] is None else i["batch"].numpy(), arith, gaps)


def test_the_fixture_holds_every_case_of_the_issue():
    for name in ("unweighted", "weighted", "directed", "edgeless_isolated", "single_graph", "duplicates_self_loops",
                 "degree_norm_off", "edge_weight_norm", "keep_self_loops", "lift_round_trip"):
        assert f"sep_{name}" in CASES, name
    assert sum(n.startswith("sep_hand_") for n in CASES) >= 5  # (a hand graph that failed a condition was left out)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_reference_labels(name):
    c = CASES[name]
    labels, k = run(c, "f64")
    assert k == c["expected"]["num_supernodes"]
    assert labels.tolist() == c["expected"]["cluster_index"].tolist()


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_arithmetic_modes_agree_and_keep_their_gaps(name):
    c = CASES[name]
    g64, gk = {}, {}
    l64, k64 = run(c, "f64", g64)
    lk, kk = run(c, "kernel", gk)
    assert k64 == kk and l64.tolist() == lk.tolist()
    assert g64.get("min_ratio", np.inf) >= 1e-5 and gk.get("min_ratio", np.inf) >= 1e-9  # what the generator kept it for


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_relabelling_the_nodes_permutes_the_partition(seed):
    g = torch.Generator().manual_seed(seed)
    n = 24
    a = torch.triu(torch.rand(n, n, generator=g) < 0.2, 1)
    ei = a.nonzero().t()
    ei = torch.cat([ei, ei.flip(0)], 1)
    w = torch.rand(n, n, generator=g) + 0.1
    w = (w + w.t())[ei[0], ei[1]]
    gaps = {}
    lab, k = R.sep_select(n, ei.numpy(), w.numpy(), None, "f64", gaps)
    assert gaps.get("min_ratio", np.inf) >= 1e-9, "not a tie-free graph: pick another seed"
    perm = torch.randperm(n, generator=g)  # node i becomes perm[i]
    lab2, k2 = R.sep_select(n, perm[ei].numpy(), w.numpy(), None, "f64")
    groups = lambda lb, idx: sorted(sorted(int(idx[i]) for i in range(n) if lb[i] == c) for c in range(k))  # noqa: E731
    assert k2 == k and groups(lab, perm) == groups(lab2, torch.arange(n))
