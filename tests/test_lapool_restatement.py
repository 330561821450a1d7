"""tests/lapool_restatement.py against the reference's fixtures, on the CPU: leader sets and shapes exact, values at
1e-5 (float32) and at float64's own precision against the stored float64 run."""
import os

import pytest
import torch

import lapool_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_lapool_v1.pt"), weights_only=True)["cases"]


def test_the_required_cases_are_stored():
    names = set(CASES)
    for mode in ("batched", "unbatched"):
        for out in ("denseout", "sparseout"):
            for kind in ("batch", "messy", "edgeless"):
                assert f"lapool_{kind}_{mode}_{out}" in names
        assert f"lapool_single_{mode}" in names and f"lapool_directed_{mode}" in names
    for name in ("lapool_dense_mask", "lapool_keep_self_loops", "lapool_no_degree_norm", "lapool_edge_weight_norm",
                 "lapool_s_inv_inverse"):
        assert name in names
    c = CASES["lapool_batch_batched_denseout"]
    sizes = torch.bincount(c["inputs"]["batch"])
    assert 4 <= sizes.numel() <= 6 and 5 <= int(sizes.min()) and int(sizes.max()) <= 40
    assert CASES["lapool_single_unbatched"]["inputs"]["batch"] is None
    ei = CASES["lapool_directed_unbatched"]["inputs"]["edge_index"]
    pairs = set(map(tuple, ei.t().tolist()))
    assert any((b, a) not in pairs for a, b in pairs)
    m = CASES["lapool_messy_unbatched_denseout"]["inputs"]
    assert bool((m["edge_index"][0] == m["edge_index"][1]).any()) and int((m["edge_weight"] == 0).sum()) == 1
    assert len(set(map(tuple, m["edge_index"].t().tolist()))) < m["edge_index"].size(1)
    e = CASES["lapool_edgeless_unbatched_denseout"]["inputs"]
    assert not bool((e["batch"][e["edge_index"][0]] == 1).any())
    deg = torch.bincount(e["edge_index"].reshape(-1), minlength=e["x"].size(0))
    assert bool(((deg == 0) & (e["batch"] != 1)).any())
    dm = CASES["lapool_dense_mask"]["inputs"]["mask"]
    assert len(set(dm.sum(1).tolist())) > 1
    assert all("seed" in c for c in CASES.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_reference(name):
    case = CASES[name]
    exp, f64 = case["expected"]["so"], case["f64"]
    _, v, lead, s = R.case_select(case, torch.float32)
    assert torch.equal(lead, exp["leader_mask"])
    assert s.shape == exp["s"].shape
    torch.testing.assert_close(s.detach(), exp["s"], rtol=1e-5, atol=1e-5)
    x64, v64, lead64, s64 = R.case_select(case, torch.float64)
    assert torch.equal(lead64, exp["leader_mask"])
    torch.testing.assert_close(v64, f64["v"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(s64.detach(), f64["s"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(v, f64["v"].float(), rtol=1e-5, atol=1e-5)


def test_structure_of_s():
    case = CASES["lapool_edgeless_batched_denseout"]
    x, v, lead, s = R.case_select(case, torch.float64)
    s = s.detach()
    k = lead.sum(1)
    for b in range(s.size(0)):
        assert torch.equal(s[b, :, int(k[b]):], torch.zeros_like(s[b, :, int(k[b]):]))
        rows = lead[b].nonzero(as_tuple=True)[0]
        assert torch.equal(s[b, rows, :int(k[b])], torch.eye(int(k[b]), dtype=s.dtype))
    real = case["expected"]["so"]["in_mask"]
    assert torch.equal(s[~real], torch.zeros_like(s[~real]))
    torch.testing.assert_close(s[real].sum(-1), torch.ones(int(real.sum()), dtype=s.dtype))


def test_ties_make_every_node_a_leader():
    n = 9
    ring = torch.stack([torch.arange(n), (torch.arange(n) + 1) % n])
    ei = torch.cat([ring, ring.flip(0)], 1)
    x = torch.ones(n, 3)
    v, lead, s = R.select(x, edge_index=ei)
    assert torch.equal(v, torch.zeros(n)) and bool(lead.all()) and torch.equal(s, torch.eye(n))


def test_zero_row_is_uniform():
    x = torch.randn(6, 3)
    x[2] = 0
    lead = torch.tensor([True, False, False, True, False, True])
    s = R.assign(x, lead)
    assert torch.equal(s[2], torch.full((3,), 1 / 3))
