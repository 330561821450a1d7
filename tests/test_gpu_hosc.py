"""HOSC pooling on the GPU.

* Fixture parity: every pooler case of tests/golden/golden_hosc_v1.pt (made by the reference, tests/golden/make_golden_hosc.py)
  at the project's rtol = atol = 1e-5: S, x, the pooled adjacency or edges (indices exact), batch and the two losses.
* Each route, forced by shape, against the float64 restatement (tests/hosc_restatement.py, which forms A A A explicitly) by
  maximum relative error.  The bound is ROUTE_REL = 1e-5, the project's fp32 tolerance: three chained reductions of at
  most 256 non-negative terms each grow fp32's unit roundoff (6e-8) to about 3 sqrt(256) 6e-8 = 3e-6.  ``hosc_loss`` is
  judged relative to itself (a ratio of same-sign sums), ``ortho_loss`` with ``hosc_ortho`` relative to
  mu sqrt(K) / (sqrt(K) - 1) (the larger of its two cancelling terms) and otherwise to itself, tensors relative to their
  max-norm.  Float64 inputs on the device run at 1e-10.
* Gradients of each loss alone, with tests/test_gpu_grad_paths.py's helper and constants, the restatement as the fp64 and
  fp32 oracle.
* The motif adjacency is never formed: the peak of allocated memory around compute_loss and its backward.
* Degenerate inputs: an edgeless graph, an all-zero column of S, alpha in {0, 1}, mu = 0.
"""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hosc_restatement as R  # noqa: E402
from test_gpu_golden import check_output, check_so  # noqa: E402
from test_gpu_grad_paths import CAP, FACTOR, FLOOR, _graphs, _linears, grad_path_errors  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = torch.load(os.path.join(HERE, "golden", "golden_hosc_v1.pt"), weights_only=True)["cases"]
POOL = sorted(k for k, v in CASES.items() if v["kind"] == "pool")
ROUTE_REL = 1e-5
F64_REL = 1e-10


def _dev():
    return torch.device("cuda:0")


def _pooler(alias, cfg):
    from tgp.poolers import HOSCPooling
    return HOSCPooling(**cfg, batched=(alias == "hosc"))


def _call(pooler, inp, dev):
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    if "adj" in d:
        return pooler(x=d["x"], adj=d["adj"], mask=d.get("mask"))
    return pooler(x=d["x"], adj=d["edge_index"], edge_weight=d.get("edge_weight"), batch=d.get("batch"))


@pytest.mark.parametrize("name", POOL)
def test_fixture_parity(name):
    c = CASES[name]
    pooler = _pooler(c["alias"], c["cfg"]).to(_dev()).eval()
    pooler.load_state_dict(c["params"])
    with torch.no_grad():
        out = _call(pooler, c["inputs"], _dev())
    check_so(out.so, c["expected"]["so"], name)
    check_output(out, c["expected"], name)
    for k in R.LOSSES:
        assert out.loss[k].dim() == 0 and out.loss[k].dtype == torch.float32 and out.loss[k].is_cuda, k


@pytest.mark.parametrize("name", ["hosc_default", "hosc_hosc_ortho", "hosc_u_default", "hosc_u_hosc_ortho", "hosc_alpha1",
                                  "hosc_u_alpha1", "hosc_dense_inputs_mask_dirty", "hosc_edgeless_graph",
                                  "hosc_u_edgeless_graph_hosc_ortho", "hosc_mlp2"])
def test_fixture_parity_under_autograd(name):
    """Training takes the operator route (reduce_connect's differentiable form + the loss Function): same values."""
    c = CASES[name]
    pooler = _pooler(c["alias"], c["cfg"]).to(_dev())
    pooler.load_state_dict(c["params"])
    out = _call(pooler, c["inputs"], _dev())
    check_output(out, c["expected"], name + ".train")
    sum(out.loss.values()).backward()
    g = pooler.selector.mlp.lins[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0


def test_public_loss_functions():
    from tgp.utils.losses import hosc_orthogonality_loss, sparse_ho_mincut_loss, unbatched_hosc_orthogonality_loss
    for tag in ("f32", "f64"):
        c = CASES[f"hosc_functions_{tag}"]
        i = {k: v.to(_dev()) for k, v in c["inputs"].items()}
        e = c["expected"]
        one = i["batch"][i["edge_index"][0]] == 0
        none = i["edge_index"][:, :0]
        got = {
            "ortho_mask": hosc_orthogonality_loss(i["s"], i["mask"]),
            "ortho_nomask": hosc_orthogonality_loss(i["s"]),
            "ortho_sum": hosc_orthogonality_loss(i["s"], i["mask"], batch_reduction="sum"),
            "ortho_k1": hosc_orthogonality_loss(i["s"][:, :, :1].contiguous(), i["mask"]),
            "unbatched_ortho": unbatched_hosc_orthogonality_loss(i["s_flat"], i["batch"]),
            "unbatched_ortho_sum": unbatched_hosc_orthogonality_loss(i["s_flat"], i["batch"], batch_reduction="sum"),
            "unbatched_ortho_nobatch": unbatched_hosc_orthogonality_loss(i["s_flat"]),
            "unbatched_ortho_k1": unbatched_hosc_orthogonality_loss(i["s_flat"][:, :1].contiguous(), i["batch"]),
            "ho_w": sparse_ho_mincut_loss(i["edge_index"], i["s_flat"], i["edge_weight"], i["batch"]),
            "ho_u": sparse_ho_mincut_loss(i["edge_index"], i["s_flat"], None, i["batch"]),
            "ho_sum": sparse_ho_mincut_loss(i["edge_index"], i["s_flat"], i["edge_weight"], i["batch"],
                                            batch_reduction="sum"),
            "ho_nobatch": sparse_ho_mincut_loss(i["edge_index"][:, one], i["s_flat"][:6], i["edge_weight"][one]),
            "ho_nobatch_sum": sparse_ho_mincut_loss(i["edge_index"][:, one], i["s_flat"][:6], i["edge_weight"][one],
                                                    batch_reduction="sum"),
            "ho_no_edges": sparse_ho_mincut_loss(none, i["s_flat"], None, i["batch"]),
            "ho_no_edges_nobatch": sparse_ho_mincut_loss(none, i["s_flat"][:6], None),
        }
        assert set(got) == set(e)
        for k, v in got.items():
            assert v.dtype == e[k].dtype and v.is_cuda, (tag, k)
            torch.testing.assert_close(v.cpu(), e[k], rtol=1e-5, atol=1e-5, msg=lambda m: f"{tag}.{k}: {m}")


# ------------------------------------------------------------------------------------------------------------ routes
def _route_case(alias, cfg, inputs, weights, biases):
    params = {}
    for i, (w, b) in enumerate(zip(weights, biases)):
        params[f"selector.mlp.lins.{i}.weight"], params[f"selector.mlp.lins.{i}.bias"] = w, b
    return {"alias": alias, "cfg": cfg, "inputs": inputs, "params": params}


def _max_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


class _Spy:
    """Counts the calls of the HOSC entry points of tgp.kernels (and the CSR product) during one pooler call."""

    NAMES = ("hosc_small", "hosc_matvec", "hosc_node_terms", "hosc_loss_terms", "spmm_csr")

    def __init__(self, monkeypatch):
        from tgp import kernels as K
        self.count = {n: 0 for n in self.NAMES}
        for n in self.NAMES:
            monkeypatch.setattr(K, n, self._wrap(n, getattr(K, n)))

    def _wrap(self, name, fn):
        def spy(*a, **kw):
            self.count[name] += 1
            return fn(*a, **kw)
        return spy


def _check_route(case, bound=ROUTE_REL, dtype=torch.float32):
    dev = _dev()
    cfg = case["cfg"]
    pooler = _pooler(case["alias"], cfg).to(dev).to(dtype).eval()
    pooler.load_state_dict({k: v.to(dtype) for k, v in case["params"].items()})
    inp = {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
           for k, v in case["inputs"].items()}
    with torch.no_grad():
        out = _call(pooler, inp, dev)
        ref, s_ref, pooled = R.pool_losses(case, torch.float64, device=dev)
    for k in R.LOSSES:
        assert out.loss[k].dtype == dtype, k
    errs = {"s": _max_rel(out.so.s, s_ref.reshape(out.so.s.shape)), "x_pool": _max_rel(out.x, pooled["x_pool"]),
            "adj_pool": _max_rel(out.edge_index, pooled["adj_pool"])}
    errs["hosc_loss"] = abs(float(out.loss["hosc_loss"]) - float(ref["hosc_loss"])) / abs(float(ref["hosc_loss"]))
    kc, mu = cfg["k"], cfg.get("mu", 0.1)
    o_scale = mu * math.sqrt(kc) / (math.sqrt(kc) - 1) if cfg.get("hosc_ortho") else abs(float(ref["ortho_loss"]))
    errs["ortho_loss"] = abs(float(out.loss["ortho_loss"]) - float(ref["ortho_loss"])) / o_scale
    print(case["alias"], cfg, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= bound, (k, v, bound)


def _sparse_case(alias, sizes, f, k, seed, directed, hosc_ortho=False, deg=4.0):
    """Directed and weighted, or undirected and unweighted (a symmetric adjacency: the backward's A = A^T shortcut)."""
    x, ei, ew, batch = _graphs(sizes, f, deg, seed, weighted=directed, directed=directed)
    ws, bs = _linears([f, k], seed + 1)
    return _route_case(alias, dict(in_channels=f, k=k, hosc_ortho=hosc_ortho),
                       dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), ws, bs)


def _dense_case(case):
    """The same graphs as already-dense padded inputs (batched mode): x [B,N,F], adj [B,N,N], mask."""
    i = case["inputs"]
    nb = int(i["batch"].max()) + 1
    w = i["edge_weight"] if i["edge_weight"] is not None else torch.ones(i["edge_index"].size(1))
    a, ptr, sizes = R.dense_blocks(i["edge_index"], w, i["batch"], nb, torch.float32)
    x = R.pad_rows(i["x"], i["batch"], ptr, nb, a.size(1))
    mask = torch.arange(a.size(1)).unsqueeze(0) < sizes.unsqueeze(1)
    # (dense inputs are read as given: adj_transpose does not transpose them, so A here is the edge list's own A)
    return dict(case, inputs=dict(x=x, adj=a, mask=mask))


SMALL = [([64, 1, 37], 4), ([20, 60], 33)]
GENERAL = [([65, 130], 20)]


@pytest.mark.parametrize("directed", [False, True], ids=["symmetric", "directed"])
@pytest.mark.parametrize("sizes,k", SMALL, ids=["n64_k4", "n60_k33"])
@pytest.mark.parametrize("hosc_ortho", [False, True], ids=["mincut_ortho", "hosc_ortho"])
def test_route_small_graph_kernel(sizes, k, directed, hosc_ortho, monkeypatch):
    """N, K <= 64: d1, d3, Z and the partial record from ONE launch in front of the tail."""
    spy = _Spy(monkeypatch)
    _check_route(_sparse_case("hosc", sizes, 6, k, 40, directed, hosc_ortho))
    assert spy.count["hosc_small"] == 1 and spy.count["hosc_matvec"] == 0 and spy.count["hosc_node_terms"] == 0
    assert spy.count["hosc_loss_terms"] == 1


@pytest.mark.parametrize("directed", [False, True], ids=["symmetric", "directed"])
@pytest.mark.parametrize("hosc_ortho", [False, True], ids=["mincut_ortho", "hosc_ortho"])
def test_route_general(directed, hosc_ortho, monkeypatch):
    """Graphs beyond 64 nodes (two row blocks, the second partly filled; K = 20 is no multiple of anything): three
    matrix-vector passes, three products, one pass over S, one tail launch."""
    spy = _Spy(monkeypatch)
    _check_route(_sparse_case("hosc", GENERAL[0][0], 6, GENERAL[0][1], 42, directed, hosc_ortho))
    assert spy.count["hosc_small"] == 0 and spy.count["hosc_matvec"] == 3
    assert spy.count["hosc_node_terms"] == 1 and spy.count["hosc_loss_terms"] == 1


@pytest.mark.parametrize("directed", [False, True], ids=["symmetric", "directed"])
def test_route_general_dense_inputs_k128(directed, monkeypatch):
    """B = 2, N = 256, K = 128 as dense inputs: two blocks of 64 columns per record, the 1024-thread tail."""
    spy = _Spy(monkeypatch)
    case = _dense_case(_sparse_case("hosc", [256, 256], 16, 128, 44, directed, hosc_ortho=directed, deg=10.0))
    _check_route(case)
    assert spy.count["hosc_small"] == 0 and spy.count["hosc_matvec"] == 3 and spy.count["hosc_node_terms"] == 1


@pytest.mark.parametrize("directed", [False, True], ids=["symmetric", "directed"])
@pytest.mark.parametrize("sizes,k,f,deg", [(SMALL[0][0], SMALL[0][1], 6, 4.0), (SMALL[1][0], SMALL[1][1], 6, 4.0),
                                           (GENERAL[0][0], GENERAL[0][1], 6, 4.0), ([256, 256], 128, 16, 10.0)],
                         ids=["n64_k4", "n60_k33", "n130_k20", "n256_k128"])
def test_route_flat(sizes, k, f, deg, directed, monkeypatch):
    """The same graphs with batched=False: three CSR products on [S | 1], the pass over the flat layout, the tail."""
    spy = _Spy(monkeypatch)
    _check_route(_sparse_case("hosc_u", sizes, f, k, 40 if deg == 4.0 else 44, directed, hosc_ortho=directed, deg=deg))
    assert spy.count["hosc_matvec"] == 0 and spy.count["hosc_small"] == 0
    assert spy.count["hosc_node_terms"] == 1 and spy.count["hosc_loss_terms"] == 1 and spy.count["spmm_csr"] >= 3


@pytest.mark.parametrize("alias", ["hosc", "hosc_u"])
def test_route_float64(alias):
    for hosc_ortho in (False, True):
        _check_route(_sparse_case(alias, GENERAL[0][0], 6, GENERAL[0][1], 46, True, hosc_ortho), bound=F64_REL,
                     dtype=torch.float64)


# --------------------------------------------------------------------------------------------------------- gradients
GRAD_CASES = [
    ("small_batched", "hosc", [9, 6, 12], 5, 4, False),
    ("small_batched_hosc_ortho", "hosc", [9, 6, 12], 5, 4, True),
    ("general_batched", "hosc", [65, 130], 6, 20, False),
    ("general_batched_hosc_ortho", "hosc", [65, 130], 6, 20, True),
    ("small_unbatched", "hosc_u", [9, 6, 12], 5, 4, True),
    ("general_unbatched", "hosc_u", [65, 130], 6, 20, False),
]


def _grad_runs(alias, sizes, f, k, seed, hosc_ortho):
    case = _sparse_case(alias, sizes, f, k, seed, True, hosc_ortho)  # directed and weighted: Zt != Z
    names = ["x"] + [n for n in case["params"]]

    def kernel():
        dev = _dev()
        pooler = _pooler(alias, case["cfg"]).to(dev)
        pooler.load_state_dict(case["params"])
        x = case["inputs"]["x"].to(dev).requires_grad_(True)
        out = _call(pooler, dict(case["inputs"], x=x), dev)
        leaves = {"x": x}
        leaves.update({f"selector.{n}": p for n, p in pooler.selector.named_parameters()})
        return dict(out.loss), leaves

    def oracle(dtype):
        ws, bs, pnames = R.selector(case["params"], dtype)
        x = case["inputs"]["x"].to(dtype).clone().requires_grad_(True)
        losses, _, _ = R.pool_losses(case, dtype, "cpu", ws, bs, x)
        leaves = {"x": x}
        leaves.update(dict(zip(pnames, [t for pair in zip(ws, bs) for t in pair])))
        return losses, leaves
    return kernel, oracle, names


@pytest.mark.parametrize("name,alias,sizes,f,k,hosc_ortho", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_gradient_paths(name, alias, sizes, f, k, hosc_ortho):
    kernel, oracle, leaves = _grad_runs(alias, sizes, f, k, 30, hosc_ortho)
    report = []
    fails = grad_path_errors(name, kernel, oracle, leaves, report=report)
    for path, leaf, e_k, e_32 in report:
        print(f"{name} | {path} | {leaf} | e_kernel {e_k:.2e} | e_oracle32 {e_32:.2e} | bound "
              f"{max(FACTOR * e_32, FLOOR):.2e} (cap {CAP:g})")
    assert report and not fails, "\n".join(fails)


@pytest.mark.parametrize("flat", [False, True], ids=["dense", "flat"])
def test_symmetric_adjacency_skips_the_transposed_chain(flat, monkeypatch):
    """An undirected unweighted batch: once kernels.AdjSymmetry knows A = A^T the backward forms no transposed product
    (Zt = Z), and its gradient equals the one of the full chain Zt = A^T (A^T (A^T S))."""
    from tgp import kernels as K
    from tgp.utils.losses import hosc_loss_terms, hosc_sparse_loss_terms
    dev = _dev()
    x, ei, _, batch = _graphs(GENERAL[0][0], 2, 4.0, 48, weighted=False, directed=False)
    g = torch.Generator().manual_seed(49)
    s_flat = torch.softmax(torch.randn(x.size(0), 7, generator=g), -1)
    a, ptr, _ = R.dense_blocks(ei, torch.ones(ei.size(1)), batch, 2, torch.float32)
    s_pad = R.pad_rows(s_flat, batch, ptr, 2, a.size(1))
    a, ei, batch = a.to(dev), ei.to(dev), batch.to(dev)
    trans, spmm = [], []
    orig_bmm, orig_spmm = K.bmm, K.spmm_csr

    def spy_bmm(p, q, trans_a=False, **kw):
        trans.append(bool(trans_a))
        return orig_bmm(p, q, trans_a=trans_a, **kw)
    monkeypatch.setattr(K, "bmm", spy_bmm)
    monkeypatch.setattr(K, "spmm_csr", lambda *p, **kw: (spmm.append(1), orig_spmm(*p, **kw))[1])

    def run():
        s = (s_flat if flat else s_pad).to(dev).clone().requires_grad_(True)
        if flat:
            terms = hosc_sparse_loss_terms(ei, None, s, batch, alpha=0.5, mu=0.0)
        else:
            terms = hosc_loss_terms(a, s, None, alpha=0.5, mu=0.0)
        torch.cuda.synchronize()  # (the verdict on the symmetry is on the host before the backward asks for it)
        del trans[:], spmm[:]
        terms.sum().backward()
        return s.grad, (sum(trans), len(spmm))
    g_short, n_short = run()
    assert n_short == (0, 0), n_short
    monkeypatch.setattr(K.AdjSymmetry, "get", lambda self: False)
    g_full, n_full = run()
    assert n_full == ((0, 3) if flat else (3, 0)), n_full
    assert _max_rel(g_short, g_full) <= ROUTE_REL


# ------------------------------------------------------------------------------------------------------------- memory
def test_motif_adjacency_is_never_formed():
    """B = 2, N = 1024, K = 16, a dense directed adjacency of 8 MB: around compute_loss and its backward the peak of
    allocated memory rises by less than ONE [B,N,N] tensor (A A and A A A would be two); the chain's own tensors are a few
    [B,N,K] of 128 KB each."""
    from tgp.poolers import HOSCPooling
    dev = _dev()
    g = torch.Generator().manual_seed(50)
    B, N, Kc = 2, 1024, 16
    adj = ((torch.rand(B, N, N, generator=g) < 0.01).float() * (torch.rand(B, N, N, generator=g) + 0.1)).to(dev)
    logits = torch.randn(B, N, Kc, generator=g).to(dev).requires_grad_(True)
    pooler = HOSCPooling(in_channels=4, k=Kc).to(dev)
    S = torch.softmax(logits, -1)
    raw = (S.transpose(1, 2) @ adj @ S).detach()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = pooler.compute_loss(adj, S, raw, None)
    (loss["hosc_loss"] + loss["ortho_loss"]).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("peak rise", rise, "bytes; one [B,N,N] tensor:", adj.numel() * 4)
    assert rise < adj.numel() * 4, (rise, adj.numel() * 4)
    assert torch.isfinite(logits.grad).all() and logits.grad.abs().sum() > 0


# --------------------------------------------------------------------------------------------------------- degenerate
def _terms_inputs(seed, B=3, N=70, Kc=5, edgeless=None):
    g = torch.Generator().manual_seed(seed)
    adj = (torch.rand(B, N, N, generator=g) < 0.1).float() * (torch.rand(B, N, N, generator=g) + 0.1)
    if edgeless is not None:
        adj[edgeless] = 0
    S = torch.softmax(torch.randn(B, N, Kc, generator=g), -1)
    return adj, S


@pytest.mark.parametrize("N", [24, 70], ids=["small_route", "general_route"])
def test_edgeless_graph_gives_zero_and_stays_finite(N):
    from tgp.utils.losses import hosc_loss_terms
    dev = _dev()
    adj, S = _terms_inputs(52, N=N, edgeless=1)
    adj, S = adj.to(dev), S.to(dev).requires_grad_(True)
    raw = (S.transpose(1, 2) @ adj @ S).detach()
    terms = hosc_loss_terms(adj, S, raw, alpha=0.5, mu=0.1, hosc_ortho=True)
    assert torch.isfinite(terms).all() and float(terms.detach()[0, 1]) == 0.0 and float(terms.detach()[0, 0]) < 0
    terms.sum().backward()
    assert torch.isfinite(S.grad).all()
    ref = 0.5 * (R.cut_terms(adj.double(), S.detach().double()) + R.ho_cut_terms(adj.double(), S.detach().double())) / 5
    assert _max_rel(terms[0], ref) <= ROUTE_REL


def test_zero_column_of_s_gets_a_zero_orthogonality_gradient():
    from tgp.utils.losses import hosc_orthogonality_loss, unbatched_hosc_orthogonality_loss
    dev = _dev()
    _, S = _terms_inputs(54)
    S[1, :, 2] = 0
    for flat in (False, True):
        s = (S[1] if flat else S).to(dev).clone().requires_grad_(True)
        loss = unbatched_hosc_orthogonality_loss(s) if flat else hosc_orthogonality_loss(s)
        loss.backward()
        assert torch.isfinite(loss) and torch.isfinite(s.grad).all()
        col = s.grad[:, 2] if flat else s.grad[1, :, 2]
        assert float(col.abs().max()) == 0.0 and float(s.grad.abs().max()) > 0
        s64 = (S[1].unsqueeze(0) if flat else S).double()
        want = R.hosc_ortho_terms(s64, s64.size(1)).mean()
        assert abs(float(loss) - float(want)) <= ROUTE_REL * math.sqrt(5) / (math.sqrt(5) - 1)


@pytest.mark.parametrize("N", [24, 70], ids=["small_route", "general_route"])
def test_alpha_and_mu_switch_their_parts_off(N, monkeypatch):
    """alpha = 0: the chain is never launched (one matrix-vector pass for the first-order degrees, no small-graph kernel);
    alpha = 1: the first-order cut is not evaluated (a poisoned raw changes nothing); mu = 0: the orthogonality row is 0."""
    from tgp.utils.losses import hosc_loss_terms
    dev = _dev()
    adj, S = _terms_inputs(56, N=N)
    adj, S = adj.to(dev), S.to(dev)
    raw = S.transpose(1, 2) @ adj @ S
    a64, s64 = adj.double(), S.double()
    spy = _Spy(monkeypatch)
    t0 = hosc_loss_terms(adj, S, raw, alpha=0.0, mu=0.0)
    assert spy.count["hosc_small"] == 0 and spy.count["hosc_matvec"] == 1
    assert _max_rel(t0[0], R.cut_terms(a64, s64) / 5) <= ROUTE_REL and float(t0[1].abs().max()) == 0.0
    t1 = hosc_loss_terms(adj, S, torch.full_like(raw, float("nan")), alpha=1.0, mu=0.2)
    assert _max_rel(t1[0], R.ho_cut_terms(a64, s64) / 5) <= ROUTE_REL
    assert _max_rel(t1[1], 0.2 * R.ortho_terms(s64)) <= ROUTE_REL
    # k: the pooler's cluster count divides the cut, whatever S's width
    t2 = hosc_loss_terms(adj, S, raw, alpha=0.25, mu=0.0, k=7)
    assert _max_rel(t2[0], (0.75 * R.cut_terms(a64, s64) + 0.25 * R.ho_cut_terms(a64, s64)) / 7) <= ROUTE_REL
    sg = S.clone().requires_grad_(True)
    hosc_loss_terms(adj, sg, raw, alpha=0.0, mu=0.0).sum().backward()
    ref = s64.clone().requires_grad_(True)
    den = (a64.sum(-1) * (ref * ref).sum(-1)).sum(-1)
    (-(torch.diagonal(raw.double(), dim1=-2, dim2=-1).sum(-1) / (den + R.EPS)) / 5).sum().backward()
    assert _max_rel(sg.grad, ref.grad) <= ROUTE_REL  # (raw is a constant here: only the degree term reaches S)
