"""The references of tests/test_gpu_rows_route_ops.py are right, and its cases are well-conditioned (no GPU needed).

* The per-graph S^T Y + postprocess_dense restatement equals oracle.dense_connect_unbatched / reduce_dense /
  postprocess_dense on a three-graph case.
* The softmax_bwd_ex formula equals autograd through torch.softmax of the same composed loss, in float64 at 1e-12.
* For every committed case the float32 run of a reference stays within CAP / FACTOR of the float64 run, per graph and
  per output: the bound max(FACTOR e_oracle32, FLOOR) of the GPU test then never needs more than CAP."""
import math

import pytest
import torch

import rows_route_refs as R
import tgp_oracle as O
from test_gpu_grad_paths import CAP, FACTOR

LIMIT = CAP / FACTOR


def _worst(ref32, ref64, blocks=None):
    return max(R.graph_errors(ref32, ref64, blocks), default=0.0)


# ------------------------------------------------------------------------------------------------------------- pins
def test_segment_products_restate_the_oracle():
    sizes, k, f = [40, 25, 33], 8, 16
    s, x, ei, ew = R.tn3_inputs(sizes, k, f, seed=1)
    s, x, ew = s.double(), x.double(), ew.double()
    batch = R.batch_of(sizes)
    raw = R.seg_tn_ref(s, R.spmm_ref(ei, ew, s), sizes)
    assert not torch.equal(raw, raw.transpose(1, 2))  # a directed list: a missed transpose shows
    torch.testing.assert_close(raw, O.dense_connect_unbatched(ei, ew, batch, s), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(R.seg_tn_ref(s, x, sizes), O.reduce_dense(s, x, batch, return_batched=True),
                               rtol=1e-12, atol=1e-14)
    for flags in R.POST_FLAGS[1:]:
        rsl, dn, adj_t, ewn = flags
        for tr in (False, True):
            m = raw.transpose(1, 2).contiguous() if tr else raw
            want = O.postprocess_dense(m, remove_self_loops=rsl, degree_norm=dn, adj_transpose=adj_t, edge_weight_norm=ewn)
            assert torch.equal(R.post_ref(raw, flags, tr), want)
    # the flags do something: the default differs from the raw matrix and from the row-sum form
    assert not torch.allclose(R.post_ref(raw, R.POST_FLAGS[2], False), raw)
    assert not torch.allclose(R.post_ref(raw, R.POST_FLAGS[2], False), R.post_ref(raw, R.POST_FLAGS[3], False))


def test_segment_nn_restates_a_block_diagonal_product():
    sizes = R.VIEW_SIZES
    g = torch.Generator().manual_seed(2)
    a = torch.randn(sum(sizes), 7, generator=g, dtype=torch.float64)
    bm = torch.randn(len(sizes), 7, 5, generator=g, dtype=torch.float64)
    want = torch.einsum("nk,nkc->nc", a, bm[R.batch_of(sizes)])
    torch.testing.assert_close(R.seg_nn_ref(a, bm, sizes), want, rtol=1e-12, atol=1e-14)
    p = R.slab_ptr(345, 40)
    assert p[0] == 0 and p[-1] == 345 and bool((p[1:] > p[:-1]).all())


@pytest.mark.parametrize("form", list(R.SOFTMAX_FORMS))
@pytest.mark.parametrize("k", [3, 17])
def test_softmax_bwd_ex_formula_is_autograd_of_the_composed_loss(form, k):
    """loss = <softmax(y), ds + extra> + sum_b c1_b sum_{i in b} deg_i |S_i|^2 + ent_g ent_scale sum -S log(S + eps):
    d loss / d y through torch.softmax is the formula, for every subset of the terms."""
    sizes, _ = R.SOFTMAX_FORMS[form]
    g = torch.Generator().manual_seed(3)
    n, eps = sum(sizes), 1e-15
    y = torch.randn(n, k, generator=g, dtype=torch.float64)
    data = R.softmax_inputs(sizes, k, seed=4)
    graph = R.batch_of(sizes)
    for terms in R.SOFTMAX_TERMS:
        a = R.softmax_args(data, terms, torch.float64)
        yl = y.clone().requires_grad_(True)
        s = torch.softmax(yl, -1)
        loss = (s * data["ds"].double()).sum()
        if a["extra"] is not None:
            loss = loss + (s * a["extra"]).sum()
        if a["c1"] is not None:
            loss = loss + (a["c1"][graph] * a["deg"] * (s * s).sum(-1)).sum()
        if a["ent_g"] is not None:
            loss = loss + a["ent_g"] * R.ENT_SCALE * (-s * torch.log(s + eps)).sum()
        loss.backward()
        got = R.softmax_bwd_ex_ref(s.detach(), data["ds"].double(), a["extra"], a["c1"], a["deg"], a["ent_g"], R.ENT_SCALE,
                                   eps, graph)
        torch.testing.assert_close(got, yl.grad, rtol=1e-12, atol=1e-12, msg=lambda m: f"{terms}: {m}")


def test_error_norm_is_per_graph_and_exact_on_zero_blocks():
    ref = torch.zeros(3, 2, 2, dtype=torch.float64)
    ref[0], ref[2] = 1000.0, 1e-3
    got = ref.clone()
    got[2, 0, 0] += 1e-4  # a small graph next to a large one is not averaged away
    e = R.graph_errors(got, ref)
    assert e[0] == 0.0 and e[1] == 0.0 and abs(e[2] - 0.1) < 1e-9
    got[1, 0, 0] = 1e-30  # a block whose reference is exactly zero must be exactly zero
    assert R.graph_errors(got, ref)[1] == math.inf
    rows = torch.ones(5, 2, dtype=torch.float64)
    assert R.graph_errors(rows, rows, blocks=[(0, 2), (2, 2), (2, 5)]) == [0.0, 0.0, 0.0]


# ----------------------------------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("name", [c[0] for c in R.TN3_CASES])
def test_tn3_cases_are_well_conditioned(name):
    sizes, k, f, s, x, ei, ew = R.tn3_case(name)
    t = R.spmm_ref(ei, ew, s)  # the float32 T is an INPUT of the operator, as on the GPU
    worst = 0.0
    raw64, raw32 = R.seg_tn_ref(s.double(), t.double(), sizes), R.seg_tn_ref(s, t, sizes)
    worst = max(worst, _worst(raw32, raw64), _worst(R.seg_tn_ref(s, x, sizes), R.seg_tn_ref(s.double(), x.double(), sizes)),
                _worst(R.seg_tn_ref(s, s, sizes), R.seg_tn_ref(s.double(), s.double(), sizes)))
    for flags in R.POST_FLAGS[1:]:
        for tr in (False, True):
            worst = max(worst, _worst(R.post_ref(raw32, flags, tr), R.post_ref(raw64, flags, tr)))
    print(f"{name}: worst e_oracle32 {worst:.2e} (limit {LIMIT:.2e})")
    assert worst <= LIMIT


@pytest.mark.parametrize("k,f", R.VIEW_KF)
def test_view_cases_are_well_conditioned(k, f):
    sizes = R.VIEW_SIZES
    blk, bm, bx = R.view_case(k, f)
    blocks = R.blocks_of(sizes)
    sv = torch.cat([blk["s"], blk["v"]], 1)
    worst = max(_worst(R.seg_nn_ref(blk["v"], bm, sizes), R.seg_nn_ref(blk["v"].double(), bm.double(), sizes), blocks),
                _worst(R.seg_nn_ref(sv, bx, sizes), R.seg_nn_ref(sv.double(), bx.double(), sizes), blocks),
                _worst((blk["v"].t() @ blk["x"])[None], (blk["v"].double().t() @ blk["x"].double())[None]),
                _worst(blk["v"].sum(0)[None], blk["v"].double().sum(0)[None]))
    print(f"views K {k} F {f}: worst e_oracle32 {worst:.2e} (limit {LIMIT:.2e})")
    assert worst <= LIMIT


def test_bmm_cases_are_well_conditioned():
    for G, M, Nc, Kd in R.BMM_SHAPES:
        a, b, c = R.bmm_case(G, M, Nc, Kd)
        assert _worst(a @ b, a.double() @ b.double()) <= LIMIT
        assert _worst(c + a @ b, c.double() + a.double() @ b.double()) <= LIMIT


@pytest.mark.parametrize("k", R.SOFTMAX_K)
def test_softmax_cases_are_well_conditioned(k):
    eps, worst = 1e-15, 0.0
    for form, (sizes, _) in R.SOFTMAX_FORMS.items():
        data = R.softmax_case(form, k)
        graph, blocks = R.batch_of(sizes), R.blocks_of(sizes)
        for terms in R.SOFTMAX_TERMS:
            r = [R.softmax_bwd_ex_ref(data["s"].to(dt), data["ds"].to(dt), **R.softmax_args(data, terms, dt),
                                      ent_scale=R.ENT_SCALE, eps=eps, graph=graph) for dt in (torch.float64, torch.float32)]
            assert torch.equal(r[0][2], torch.zeros(k, dtype=torch.float64))  # the all-zero row of S
            worst = max(worst, _worst(r[1], r[0], blocks))
    print(f"softmax_bwd_ex K {k}: worst e_oracle32 {worst:.2e} (limit {LIMIT:.2e})")
    assert worst <= LIMIT
