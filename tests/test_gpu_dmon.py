"""DMoN pooling on the GPU.

* Fixture parity: every pooler case of tests/golden/golden_dmon_v1.pt (made by the reference, tests/golden/make_golden_dmon.py)
  at the project's rtol = atol = 1e-5: S, x, the pooled adjacency or edges (indices exact), batch and the three losses.
* Each route, forced by shape, against the float64 restatement (tests/dmon_restatement.py) by maximum relative error.  The
  bound is ROUTE_REL = 1e-5, the project's fp32 tolerance: fp32's unit roundoff (6e-8) times the longest reduction here
  (1024 rows) grown as its square root is 2e-6, and the sums run over non-negative terms.  Tensors are judged relative to
  their max-norm, the spectral loss relative to trace(raw) / 2m and the cluster loss relative to ||S^T 1|| sqrt(K) / n (the
  larger of each loss's two cancelling terms); the orthogonality loss relative to itself.
* Gradients of each loss alone, with tests/test_gpu_grad_paths.py's helper and constants, the restatement as the fp64 and
  fp32 oracle.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dmon_restatement as R  # noqa: E402
from test_gpu_golden import check_output, check_so  # noqa: E402
from test_gpu_grad_paths import CAP, FACTOR, FLOOR, _graph_names, _graphs, _linears, grad_path_errors  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = torch.load(os.path.join(HERE, "golden", "golden_dmon_v1.pt"), weights_only=True)["cases"]
POOL = sorted(k for k, v in CASES.items() if v["kind"] == "pool")
ROUTE_REL = 1e-5
F64_REL = 1e-10


def _dev():
    return torch.device("cuda:0")


def _pooler(alias, cfg):
    from tgp.poolers import DMoNPooling
    return DMoNPooling(**cfg, batched=(alias == "dmon"))


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
        assert out.loss[k].dim() == 0 and out.loss[k].dtype == torch.float32, k


@pytest.mark.parametrize("name", ["dmon_batched_default_w", "dmon_batched_ortho1_w", "dmon_u_directed_w",
                                  "dmon_dense_inputs_mask_dirty", "dmon_edgeless_graph_w"])
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
    from tgp.utils.losses import cluster_loss, sparse_spectral_loss, spectral_loss, unbatched_cluster_loss
    for tag in ("f32", "f64"):
        c = CASES[f"dmon_functions_{tag}"]
        i = {k: v.to(_dev()) for k, v in c["inputs"].items()}
        e = c["expected"]
        one = i["batch"][i["edge_index"][0]] == 0
        got = {
            "spectral_mask": spectral_loss(i["adj"], i["s"], i["raw"], i["mask"]),
            "spectral_nomask": spectral_loss(i["adj"], i["s"], i["raw"]),
            "cluster_mask": cluster_loss(i["s"], mask=i["mask"]),
            "cluster_nomask": cluster_loss(i["s"]),
            "cluster_sum": cluster_loss(i["s"], mask=i["mask"], batch_reduction="sum"),
            "sparse_spectral_w": sparse_spectral_loss(i["edge_index"], i["s_flat"], i["edge_weight"], i["batch"]),
            "sparse_spectral_u": sparse_spectral_loss(i["edge_index"], i["s_flat"], None, i["batch"]),
            "sparse_spectral_nobatch": sparse_spectral_loss(i["edge_index"][:, one], i["s_flat"][:6],
                                                            i["edge_weight"][one]),
            "unbatched_cluster": unbatched_cluster_loss(i["s_flat"], i["batch"]),
            "unbatched_cluster_nobatch": unbatched_cluster_loss(i["s_flat"]),
        }
        for k, v in got.items():
            assert v.dtype == e[k].dtype, (tag, k)
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


def _check_route(case, bound=ROUTE_REL, dtype=torch.float32):
    dev = _dev()
    pooler = _pooler(case["alias"], case["cfg"]).to(dev).to(dtype).eval()
    pooler.load_state_dict({k: v.to(dtype) for k, v in case["params"].items()})
    inp = {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
           for k, v in case["inputs"].items()}
    with torch.no_grad():
        out = _call(pooler, inp, dev)
        ref, spec_scale, s_ref, pooled = R.pool_losses(case, torch.float64, device=dev)
    for k in R.LOSSES:
        assert out.loss[k].dtype == dtype, k
    errs = {"s": _max_rel(out.so.s, s_ref.reshape(out.so.s.shape)), "x_pool": _max_rel(out.x, pooled["x_pool"]),
            "adj_pool": _max_rel(out.edge_index, pooled["adj_pool"])}
    errs["spectral_loss"] = abs(float(out.loss["spectral_loss"]) - float(ref["spectral_loss"])) / float(spec_scale)
    clu_scale = abs(float(ref["cluster_loss"]) + case["cfg"].get("cluster_loss_coeff", 1.0))
    errs["cluster_loss"] = abs(float(out.loss["cluster_loss"]) - float(ref["cluster_loss"])) / clu_scale
    errs["ortho_loss"] = abs(float(out.loss["ortho_loss"]) - float(ref["ortho_loss"])) / abs(float(ref["ortho_loss"]))
    print(case.get("name", ""), {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= bound, (k, v, bound)


def _sparse_case(alias, sizes, f, k, seed, deg=4.0, weighted=True, directed=False):
    x, ei, ew, batch = _graphs(sizes, f, deg, seed, weighted, directed=directed)
    ws, bs = _linears([f, k], seed + 1)
    return _route_case(alias, dict(in_channels=f, k=k, ortho_loss_coeff=1.0),
                       dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), ws, bs)


def test_route_small_padded_batch(monkeypatch):
    """Dense padded inputs of small graphs that the one-wave-per-graph kernel takes (B >= 64, N <= 64, K and F <= 32):
    the one-launch Select + Reduce + Connect with raw and without MinCut's terms, the loss kernels behind it."""
    from tgp import kernels as K
    calls = []
    orig = K.dense_pool_select

    def spy(*a, **kw):
        calls.append((kw.get("want_raw"), kw.get("mincut_terms")))
        return orig(*a, **kw)
    monkeypatch.setattr(K, "dense_pool_select", spy)
    g = torch.Generator().manual_seed(5)
    B, N, F, Kc = 96, 24, 8, 6
    assert K.dense_pool_is_small(B, N, Kc, F)
    a = (torch.rand(B, N, N, generator=g) < 0.2).float() * (torch.rand(B, N, N, generator=g) + 0.1)
    mask = torch.arange(N).unsqueeze(0) < torch.randint(10, N + 1, (B, 1), generator=g)
    x = torch.randn(B, N, F, generator=g) * mask.unsqueeze(-1)
    ws, bs = _linears([F, Kc], 6)
    _check_route(_route_case("dmon", dict(in_channels=F, k=Kc, ortho_loss_coeff=1.0),
                             dict(x=x, adj=a * mask.unsqueeze(1) * mask.unsqueeze(2), mask=mask), ws, bs))
    assert calls == [(True, False)]


@pytest.mark.parametrize("adj_transpose,deg", [(True, 4.0), (False, 4.0), (True, 14.0)])
def test_route_small_sparse_batch(adj_transpose, deg, monkeypatch):
    """A sorted batch of small graphs as PyG hands it over: the one-launch sparse kernel with raw, the degrees from the
    edge list (in-degrees when adj_transpose), no dense adjacency.  deg = 14: graphs of more than 256 edges, so the
    degree kernel stages a graph's edges through LDS in several chunks."""
    from tgp import kernels as K
    calls, dense = [], []
    orig, orig_dense = K.dmon_edge_degrees, K.dmon_dense_terms

    def spy(*a, **kw):
        calls.append(a[-1])
        return orig(*a, **kw)

    def spy_dense(*a, **kw):
        dense.append(a[0] is not None)
        return orig_dense(*a, **kw)
    monkeypatch.setattr(K, "dmon_edge_degrees", spy)
    monkeypatch.setattr(K, "dmon_dense_terms", spy_dense)
    g = torch.Generator().manual_seed(7)
    sizes = torch.randint(20, 61, (256,), generator=g).tolist()
    case = _sparse_case("dmon", sizes, 32, 20, 8, deg=deg, directed=True)
    case["cfg"]["adj_transpose"] = adj_transpose
    per_graph = torch.bincount(case["inputs"]["batch"][case["inputs"]["edge_index"][0]])
    if deg > 4.0:
        assert int(per_graph.max()) > 256
    _check_route(case)
    assert calls == [adj_transpose] and dense == [False]  # (no pass over a dense adjacency)


def test_route_c2_dense_batch():
    """B=32, N=1024, K=128, F=64 padded dense inputs: the operator route (reduce_connect with raw) + the loss kernels."""
    g = torch.Generator().manual_seed(9)
    B, N, F, Kc = 32, 1024, 64, 128
    a = (torch.rand(B, N, N, generator=g) < 0.01).float()
    a = ((a + a.transpose(1, 2)) > 0).float()
    x = torch.randn(B, N, F, generator=g)
    ws, bs = _linears([F, Kc], 10)
    _check_route(_route_case("dmon", dict(in_channels=F, k=Kc, ortho_loss_coeff=1.0), dict(x=x, adj=a), ws, bs))


def test_route_large_sparse_batch_declines_rows_route(monkeypatch):
    """Large sparse graphs: the rows route declines DMoN (no native call hands out raw without a MinCut/DiffPool tail
    there), the batch is densified and takes the operator route: reduce_connect with raw, then one pass over the dense
    adjacency for the degrees."""
    from tgp import kernels as K
    from tgp.poolers import _DenseMLPPooling
    taken, dense, pooled = [], [], []
    orig, orig_dense, orig_pool = _DenseMLPPooling._unbatched_fused, K.dmon_dense_terms, K.dense_pool

    def spy(self, *a, **kw):
        r = orig(self, *a, **kw)
        taken.append(r is not None)
        return r

    def spy_dense(*a, **kw):
        dense.append(tuple(a[0].shape) if a[0] is not None else None)
        return orig_dense(*a, **kw)

    def spy_pool(*a, **kw):
        if a[1] is not None:  # (the Connect product; S^T S passes no adjacency)
            pooled.append(kw.get("want_raw"))
        return orig_pool(*a, **kw)
    monkeypatch.setattr(_DenseMLPPooling, "_unbatched_fused", spy)
    monkeypatch.setattr(K, "dmon_dense_terms", spy_dense)
    monkeypatch.setattr(K, "dense_pool", spy_pool)
    sizes = [700, 512, 650, 600]
    _check_route(_sparse_case("dmon", sizes, 32, 32, 12, deg=6.0))
    assert taken and not any(taken)
    assert dense == [(4, 700, 700)] and pooled == [True]


def test_route_unbatched():
    _check_route(_sparse_case("dmon_u", [200, 256, 180], 16, 32, 14))


def test_route_directed_both_modes():
    for alias in ("dmon", "dmon_u"):
        _check_route(_sparse_case(alias, [90, 60, 120], 8, 8, 16, directed=True))


def test_route_float64():
    for alias in ("dmon", "dmon_u"):
        _check_route(_sparse_case(alias, [90, 60, 120], 8, 8, 18), bound=F64_REL, dtype=torch.float64)


# --------------------------------------------------------------------------------------------------------- gradients
GRAD_CASES = [
    ("small_batched", "dmon", [9, 6, 12], 5, 4),
    ("medium_batched", "dmon", [200, 256, 180], 16, 32),
    ("small_unbatched", "dmon_u", [9, 6, 12], 5, 4),
    ("medium_unbatched", "dmon_u", [200, 256, 180], 16, 32),
    ("directed_batched", "dmon", [40, 30, 50], 8, 8),
    # 64 graphs: the batch the one-wave-per-graph kernel takes -- the fused Reduce + Connect Function hands the loss a
    # differentiable raw and receives its gradient (test_small_batch_trains_through_the_fused_function)
    ("small_batch_64", "dmon", [10 + (i * 7) % 11 for i in range(64)], 5, 4),
]


def _grad_runs(alias, sizes, f, k, seed, directed=False):
    case = _sparse_case(alias, sizes, f, k, seed, directed=directed)
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
        losses, _, _, _ = R.pool_losses(case, dtype, "cpu", ws, bs, x)
        leaves = {"x": x}
        leaves.update(dict(zip(pnames, [t for pair in zip(ws, bs) for t in pair])))
        return losses, leaves
    return kernel, oracle, names


@pytest.mark.parametrize("name,alias,sizes,f,k", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_gradient_paths(name, alias, sizes, f, k):
    kernel, oracle, leaves = _grad_runs(alias, sizes, f, k, 30, directed=name.startswith("directed"))
    report = []
    fails = grad_path_errors(name, kernel, oracle, leaves, report=report)
    for path, leaf, e_k, e_32 in report:
        print(f"{name} | {path} | {leaf} | e_kernel {e_k:.2e} | e_oracle32 {e_32:.2e} | bound "
              f"{max(FACTOR * e_32, FLOOR):.2e} (cap {CAP:g})")
    assert not fails, "\n".join(fails)


def test_small_batch_trains_through_the_fused_function():
    """Training on 64 small graphs: the losses' raw comes from the fused Reduce + Connect Function (its backward takes
    the gradient of raw), behind the DMoN loss Function."""
    name, alias, sizes, f, k = GRAD_CASES[-1]
    case = _sparse_case(alias, sizes, f, k, 30)
    dev = _dev()
    pooler = _pooler(alias, case["cfg"]).to(dev)
    pooler.load_state_dict(case["params"])
    x = case["inputs"]["x"].to(dev).requires_grad_(True)
    out = _call(pooler, dict(case["inputs"], x=x), dev)
    names = _graph_names(out.loss["spectral_loss"].grad_fn)
    assert "_DMoNTermsFnBackward" in names and "_DensePoolSmallFnBackward" in names, names
