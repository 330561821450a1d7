"""The NMF restatement (tests/nmf_restatement.py) against the reference's stored results
(tests/golden/golden_nmf_v1.pt): scikit-learn's coordinate descent from the recorded init, iteration counts included."""
import os

import pytest
import torch

import nmf_restatement as R
import tgp_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
BLOB = torch.load(os.path.join(HERE, "golden", "golden_nmf_v1.pt"), weights_only=True)
CASES, OPTS = BLOB["cases"], BLOB["opts"]
TOL = dict(rtol=1e-5, atol=1e-5)


def test_the_required_cases_are_stored():
    assert BLOB["tgp_version"] == "1.0.1" and len(OPTS) == 3
    singles = [c for c in CASES.values() if c["single"]]
    assert any(c["k"] < c["sizes"][0] for c in singles) and any(c["k"] == c["sizes"][0] for c in singles)
    assert any(c["k"] > c["sizes"][0] and not c["fixed_k"] for c in singles) and any(c["fixed_k"] for c in singles)
    mixed = CASES["nmf_batch_mixed"]
    k, sizes = mixed["k"], mixed["sizes"]
    assert 1 in sizes and 2 in sizes and any(2 < m <= k for m in sizes) and any(m > k for m in sizes)
    i = mixed["inputs"]
    eb = i["batch"][i["edge_index"][0]]
    assert any(int((eb == g).sum()) == 0 and m > k for g, m in enumerate(sizes))  # a factorised graph without edges
    key = i["edge_index"][0] * i["batch"].numel() + i["edge_index"][1]
    assert key.unique().numel() < key.numel() and bool((i["edge_weight"] < 0).any())  # duplicates, negative weights
    lo = 0
    asym = []
    for m in sizes:
        a = R.dense_adjacency(i["edge_index"], i["edge_weight"], lo, lo + m)
        asym.append(not torch.equal(a, a.t()))
        lo += m
    assert any(asym)  # a directed graph
    for c in CASES.values():  # the margins that make the counts safe in fp32
        for gi, it in enumerate(c["sklearn_iter"]):
            assert c["err_ref"][gi] <= 2.5e-6 and c["f64"]["iters"][gi] == it
            if it > 1:
                assert c["f64"]["ratio_last"][gi] <= 0.98 * c["tol"] and c["f64"]["ratio_prev"][gi] >= 1.02 * c["tol"]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_reference(name, dtype):
    c = CASES[name]
    i, want = c["inputs"], c["expected"]
    n = i["x"].size(0)
    got = R.nmf_select(i["edge_index"], c["k"], i["edge_weight"], i["batch"], n, fixed_k=c["fixed_k"], tol=c["tol"],
                       max_iter=c["max_iter"], init=(c["w0"], c["h0t"]), dtype=dtype)
    assert tuple(got["s"].shape) == tuple(want["s"].shape)
    torch.testing.assert_close(got["s"].float(), want["s"], **TOL)
    assert got["iters"] == c["sklearn_iter"]
    if dtype == torch.float64:
        # the stored float64 run again, on another machine's BLAS: the products' summation order may differ, so not bit
        # for bit.  fp32 against float64 differs by err_ref <= 1.6e-7 here, 3 x fp32's 2^-24; float64's 2^-53 with the
        # same amplification is 3e-16 (seen: 6e-16), and 1e-12 leaves three orders of magnitude over that
        torch.testing.assert_close(got["s"], c["f64"]["s"], rtol=1e-12, atol=1e-12)
        return
    # x_pool, adj_pool (the dense option sets) and lift from this S through the oracle's dense operators
    s, x, b = got["s"], i["x"], i["batch"]
    x_pool = O.reduce_dense(s, x, b, return_batched=True)
    torch.testing.assert_close(x_pool.reshape(want["x_pool"].shape), want["x_pool"], **TOL)
    raw = O.dense_connect_unbatched(i["edge_index"], i["edge_weight"], b, s)
    for oi, opts in enumerate(OPTS):
        if opts["sparse_output"]:
            continue
        # (the reference's unbatched DenseConnect sums the degrees along the last axis whatever adj_transpose says)
        adj = O.postprocess_dense(raw, opts["remove_self_loops"], opts["degree_norm"], False, opts["edge_weight_norm"])
        torch.testing.assert_close(adj, want["adj"][oi]["dense"], **TOL)
    parts = s.split(c["sizes"])
    lift = torch.cat([sg @ xp for sg, xp in zip(parts, x_pool)])
    torch.testing.assert_close(lift, want["lift"], **TOL)


def test_special_cases_and_widths():
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    w = torch.tensor([0.5, 0.5, 0.25, 0.25])
    assert tuple(R.nmf_select(torch.zeros(2, 0, dtype=torch.long), 3)["s"].shape) == (0, 0)
    assert tuple(R.nmf_select(torch.zeros(2, 0, dtype=torch.long), 3, fixed_k=True)["s"].shape) == (0, 3)
    assert torch.equal(R.nmf_select(ei, 3, w)["s"], torch.eye(3))  # k = n
    assert torch.equal(R.nmf_select(ei, 5, w)["s"], torch.eye(3))  # k > n: width n
    assert torch.equal(R.nmf_select(ei, 5, w, fixed_k=True)["s"], torch.cat([torch.eye(3), torch.zeros(3, 2)], 1))
    assert torch.equal(R.nmf_select(ei, 1, w)["s"], torch.ones(3, 1))
    one = R.nmf_select(torch.zeros(2, 0, dtype=torch.long), 4, num_nodes=1)
    assert torch.equal(one["s"], torch.ones(1, 1)) and one["iters"] == [0]
    batch = torch.tensor([0, 0, 0, 1, 2, 2])
    got = R.nmf_select(ei, 2, w, batch)
    assert tuple(got["s"].shape) == (6, 2) and got["iters"][1:] == [0, 0] and got["iters"][0] > 0
    assert torch.equal(got["s"][3:], torch.tensor([[1.0, 0], [1.0, 0], [0, 1.0]]))


def test_all_zero_adjacency_is_uniform_after_one_iteration():
    for dtype in (torch.float32, torch.float64):
        got = R.nmf_select(torch.zeros(2, 0, dtype=torch.long), 3, num_nodes=7, dtype=dtype)
        assert got["iters"] == [1] and got["ratios"] == [[0.0]]
        assert torch.equal(got["s"], torch.full((7, 3), 1.0 / 3.0, dtype=dtype))
    # negative weights only: clamped to the same thing
    ei = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 0]])
    got = R.nmf_select(ei, 2, -torch.ones(4), num_nodes=4)
    assert got["iters"] == [1] and torch.equal(got["s"], torch.full((4, 2), 0.5))


def test_default_init_range_and_independence_of_graph_position():
    u = R.hash_uniform(5, 0, 64, 16)
    assert float(u.min()) > 0.0 and float(u.max()) <= 1.0 and u.unique().numel() > 1000
    assert torch.equal(u * 16777216.0, (u * 16777216.0).round())  # multiples of 2^-24: exact in fp32
    assert not torch.equal(u, R.hash_uniform(5, 1, 64, 16)) and not torch.equal(u, R.hash_uniform(6, 0, 64, 16))
    assert torch.equal(R.hash_uniform(5, 0, 10, 4), u[:10, :4])  # a function of (seed, which, i, t) alone
    assert abs(float(u.mean()) - 0.5) < 0.05
    ei, ew, batch = R.planted_graphs([[4, 4], [5, 4, 3], [4, 4]], 3)
    a = R.dense_adjacency(ei, ew, 8, 20)
    w0, h0t = R.default_init(a, 3, 7)
    avg = float(torch.sqrt(a.mean() / 3))
    for f in (w0, h0t):
        assert f.dtype == torch.float32 and float(f.min()) > 0.0 and float(f.max()) <= 2.0 * avg
    # the same graph first in one batch and last in another: the same rows
    n1 = int((batch == 1).sum())
    e1 = batch[ei[0]] == 1
    solo_ei, solo_w = ei[:, e1] - 8, ew[e1]
    alone = R.nmf_select(solo_ei, 3, solo_w, num_nodes=n1, seed=7)
    inside = R.nmf_select(ei, 3, ew, batch, seed=7)
    assert torch.equal(inside["s"][8:20], alone["s"]) and inside["iters"][1] == alone["iters"][0]
    shifted_ei = torch.cat([ei[:, batch[ei[0]] == 0], solo_ei + 8], 1)
    shifted = R.nmf_select(shifted_ei, 3, torch.cat([ew[batch[ei[0]] == 0], solo_w]),
                           torch.tensor([0] * 8 + [1] * n1), seed=7)
    assert torch.equal(shifted["s"][8:], alone["s"])
    assert not torch.equal(R.nmf_select(solo_ei, 3, solo_w, num_nodes=n1, seed=8)["s"], alone["s"])
