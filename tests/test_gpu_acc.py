"""AsymCheegerCut pooling on the GPU.

* Fixture parity: every case of tests/golden/golden_acc_v1.pt (made by the reference, tests/golden/make_golden_acc.py) at
  the project's rtol = atol = 1e-5, through the pooler and through the four loss functions; Select / Reduce / Connect
  equal MinCutPooling's on the same parameters and inputs.
* The quantile select against ``torch.sort`` bit for bit, on both of its routes.
* Values and gradients against the float64 restatement (tests/acc_restatement.py) at float32's own error: the bound is
  FACTOR times the error of the float32 torch restatement against the float64 one on the same inputs (floor FLOOR), the
  constants and the helper of tests/test_gpu_grad_paths.py.
* Bitwise determinism, every row of the route table, and two scale cases.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import acc_restatement as R  # noqa: E402
from test_acc_restatement import function_values  # noqa: E402
from test_gpu_golden import check_output, check_so  # noqa: E402
from test_gpu_grad_paths import CAP, FACTOR, FLOOR, _graph_names, _graphs, _linears, grad_path_errors  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = torch.load(os.path.join(HERE, "golden", "golden_acc_v1.pt"), weights_only=True)["cases"]
POOL = sorted(k for k, v in CASES.items() if v["kind"] == "pool")
ONE_NODE = ("_SelectPoolSmallFnBackward", "_SelectPoolSparseFnBackward", "_PoolLargeFnBackward", "_PoolUnbatchedFnBackward")


def _dev():
    return torch.device("cuda:0")


def _pooler(alias, cfg, cls=None):
    from tgp.poolers import AsymCheegerCutPooling
    return (cls or AsymCheegerCutPooling)(**cfg, batched=not alias.endswith("_u"))


def _call(pooler, inp, dev):
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    if "adj" in d:
        return pooler(x=d["x"], adj=d["adj"], mask=d.get("mask"))
    return pooler(x=d["x"], adj=d["edge_index"], edge_weight=d.get("edge_weight"), batch=d.get("batch"))


# ------------------------------------------------------------------------------------------------------------ parity
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
    assert set(out.loss) == set(R.LOSSES)


@pytest.mark.parametrize("name", ["acc_batched_default_w", "acc_u_directed_w", "acc_dense_inputs_mask",
                                  "acc_edgeless_graph_w", "acc_u_zero_weight_edges", "acc_n_lt_k"])
def test_fixture_parity_under_autograd(name):
    c = CASES[name]
    pooler = _pooler(c["alias"], c["cfg"]).to(_dev())
    pooler.load_state_dict(c["params"])
    out = _call(pooler, c["inputs"], _dev())
    check_output(out, c["expected"], name + ".train")
    sum(out.loss.values()).backward()
    g = pooler.selector.mlp.lins[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0


@pytest.mark.parametrize("name", ["acc_batched_default_w", "acc_batched_noT_ewn_u", "acc_unbatched_default_w",
                                  "acc_dense_inputs_mask", "acc_batched_sparse_out_w"])
def test_select_reduce_connect_are_mincut_s(name):
    from tgp.poolers import MinCutPooling
    c = CASES[name]
    cfg = {k: v for k, v in c["cfg"].items() if k not in ("totvar_coeff", "balance_coeff")}
    outs = []
    for cls in (None, MinCutPooling):
        pooler = _pooler(c["alias"], cfg, cls).to(_dev()).eval()
        pooler.load_state_dict(c["params"])
        with torch.no_grad():
            outs.append(_call(pooler, c["inputs"], _dev()))
    a, m = outs
    for got, want in ((a.x, m.x), (a.so.s, m.so.s), (a.edge_index, m.edge_index), (a.edge_weight, m.edge_weight)):
        if want is None:
            assert got is None
        elif want.dtype == torch.long:
            assert torch.equal(got, want)
        else:
            torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


class Device:
    """The package's public functions on device tensors, per call reduced to one value (as function_values asks)."""

    @staticmethod
    def totvar(adj, S):
        from tgp.utils.losses import totvar_loss
        return totvar_loss(S, adj).reshape(1)

    @staticmethod
    def asym(S, k, mask=None):
        from tgp.utils.losses import asym_norm_loss
        return asym_norm_loss(S, k, mask=mask).reshape(1)

    @staticmethod
    def sparse_totvar(edge_index, S, w, batch, nb):
        from tgp.utils.losses import sparse_totvar_loss
        return sparse_totvar_loss(edge_index, S, w, batch).reshape(1)

    @staticmethod
    def unbatched_asym(S, k, batch, nb):
        from tgp.utils.losses import unbatched_asym_norm_loss
        return unbatched_asym_norm_loss(S, k, batch).reshape(1)


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_public_loss_functions(tag):
    from tgp.utils.losses import asym_norm_loss, totvar_loss
    c = CASES[f"acc_functions_{tag}"]
    i = {k: v.to(_dev()) for k, v in c["inputs"].items()}
    e = c["expected"]
    got = function_values(Device, i, int(i["batch"].max()) + 1)
    got["totvar_sum"] = totvar_loss(i["s"], i["adj"], batch_reduction="sum")
    got["asym_sum"] = asym_norm_loss(i["s"], i["s"].size(-1), mask=i["mask"], batch_reduction="sum")
    assert set(got) == set(e)
    for k, v in got.items():
        assert v.dtype == e[k].dtype, (tag, k)
        torch.testing.assert_close(v.cpu(), e[k], rtol=1e-5, atol=1e-5, msg=lambda m: f"{tag}.{k}: {m}")


# ---------------------------------------------------------------------------------------------------------- quantile
def _special_columns(n, g):
    """[n, 12] float32: columns that are hard for a selection by bits."""
    tiny = torch.tensor(1e-41)  # a denormal
    cols = [
        torch.randn(n, generator=g),                                             # plain
        torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0)),  # +-0 only
        torch.randn(n, generator=g).round() * 0.0 + torch.randint(-1, 2, (n,), generator=g) * 0.0,  # signed zeros
        torch.randint(-3, 4, (n,), generator=g).float() * tiny,                 # denormals of both signs and zeros
        torch.full((n,), 0.25),                                                  # constant
        (torch.rand(n, generator=g) < 0.3).float(),                              # saturated to exact 0.0 / 1.0
        torch.randint(0, 4, (n,), generator=g).float() / 3,                      # many ties
        -torch.rand(n, generator=g),                                             # all negative
        torch.softmax(torch.randn(n, 8, generator=g) * 30, -1)[:, 0],            # a saturated softmax column
        torch.randn(n, generator=g) * 1e30,                                      # large magnitudes
        torch.arange(n).float(),                                                 # ascending
        -torch.arange(n).float(),                                                # descending
    ]
    return torch.stack(cols, 1)


def _check_quantile(s, k, got, rows_of):
    """``got`` of K.acc_quantile against torch.sort per graph; ``rows_of(b)`` = the real row indices of graph b."""
    q, qnode, colsum, cge, nreal, _ = got
    for b in range(q.size(0)):
        idx_rows = rows_of(b)
        rows = s[b][idx_rows] if s.dim() == 3 else s[idx_rows]
        n = rows.size(0)
        assert int(nreal[b]) == n
        if n == 0:
            assert bool((qnode[b] == -1).all())
            continue
        idx = min(n // k, n - 1)
        want = torch.sort(rows, dim=0, descending=True)[0][idx]
        # bit for bit; -0 and +0 are one value to a sort, so both sides are compared with their zeros made +0
        zero = torch.zeros_like(want)
        assert torch.equal(torch.where(q[b] == 0, zero, q[b]).view(torch.int32),
                           torch.where(want == 0, zero, want).view(torch.int32)), b
        first = (rows == want).to(torch.int64).argmax(0)
        local = qnode[b].long()
        base = idx_rows[0] if s.dim() == 2 else 0
        assert torch.equal(idx_rows[first] - base, local), (b, idx_rows[first] - base, local)
        picked = rows[first, torch.arange(rows.size(1), device=s.device)]
        assert torch.equal(q[b].view(torch.int32), picked.view(torch.int32)), b  # (the node's own bits)
        d = rows.double() - want.double()
        assert torch.equal(cge[b].long(), (d >= 0).sum(0))
        ref = torch.where(d >= 0, (k - 1) * d, -d).sum(0)
        torch.testing.assert_close(colsum[b].double(), ref, rtol=1e-4, atol=1e-30)


@pytest.mark.parametrize("n,route", [(100, "count"), (37, "count"), (128, "count"), (129, "radix"), (333, "radix"),
                                     (1000, "radix")])
def test_quantile_select_is_exact_on_both_routes(n, route):
    from tgp import kernels as K
    dev = _dev()
    g = torch.Generator().manual_seed(n)
    B = 3
    s = torch.stack([_special_columns(n, g) for _ in range(B)]).to(dev)
    k = 7
    got = K.acc_quantile(s, k)
    assert got[-1] == route and (n <= K.acc_small_graph_nodes()) == (route == "count")
    _check_quantile(s, k, got, lambda b: torch.arange(n, device=dev))
    # a mask that is not a prefix, and graph sizes
    mask = torch.rand(B, n, generator=g) < 0.7
    mask[1] = False
    mask[1, 5] = True  # (a graph of one real node)
    mask = mask.to(dev)
    got = K.acc_quantile(s, k, mask=mask)
    assert got[-1] == route
    _check_quantile(s, k, got, lambda b: mask[b].nonzero().view(-1))
    sizes = torch.tensor([n, n // 3, 0], device=dev)
    got = K.acc_quantile(s, k, graph_sizes=sizes)
    _check_quantile(s, k, got, lambda b: torch.arange(int(sizes[b]), device=dev))
    # the un-padded layout, graphs of different lengths (the longest decides the route)
    ptr = torch.tensor([0, n // 4, n // 4, n // 4 + n], device=dev)
    flat = s.reshape(-1, s.size(-1))[: int(ptr[-1])].contiguous()
    got = K.acc_quantile(flat, k, ptr=ptr, max_nodes=n)
    assert got[-1] == route
    _check_quantile(flat, k, got, lambda b: torch.arange(int(ptr[b]), int(ptr[b + 1]), device=dev))
    # the radix select on what the counting select took: the same bits
    if route == "count":
        a, b_ = K.acc_quantile(s, k, mask=mask), K.acc_quantile(s, k, mask=mask, route="radix")
        assert a[-1] == "count" and b_[-1] == "radix"
        for x, y in zip(a[:5], b_[:5]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_quantile_select_many_columns_and_k_values():
    from tgp import kernels as K
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    for n, cols, k in ((50, 70, 2), (50, 70, 60), (700, 130, 128), (700, 33, 3)):
        s = torch.softmax(torch.randn(2, n, cols, generator=g), -1).to(dev)
        _check_quantile(s, k, K.acc_quantile(s, k), lambda b: torch.arange(n, device=dev))


# -------------------------------------------------------------------------------------------- values at fp32's own error
def _bound(f32, f64):
    e32 = abs(float(f32) - float(f64)) / max(abs(float(f64)), 1e-300)
    return max(FACTOR * e32, FLOOR), e32


def _check_value(name, got, f32, f64):
    bound, e32 = _bound(f32, f64)
    err = abs(float(got) - float(f64)) / max(abs(float(f64)), 1e-300)
    print(f"{name}: kernel {float(got):.9g} f64 {float(f64):.9g} e_kernel {err:.2e} e_oracle32 {e32:.2e} bound {bound:.2e}")
    assert bound <= CAP and err <= bound, (name, err, bound)


def _dense_batch(B, N, K, density, seed, weighted=False, symmetric=True):
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(B, N, N, generator=g) < density).float()
    if symmetric:
        a = ((a + a.transpose(1, 2)) > 0).float()
    if weighted:
        a = a * (torch.rand(B, N, N, generator=g) + 0.25)
    s = torch.softmax(torch.randn(B, N, K, generator=g), -1)
    return a, s


@pytest.mark.parametrize("name,B,N,K,density", [("dense", 2, 200, 24, 1.1), ("one_percent", 3, 1024, 32, 0.01),
                                                ("odd_n", 2, 203, 70, 0.05), ("wide_k", 1, 96, 300, 0.2)])
def test_totvar_dense_values(name, B, N, K, density):
    from tgp.utils.losses import totvar_loss
    a, s = _dense_batch(B, N, K, density, 41, weighted=True, symmetric=False)
    if name == "one_percent":
        a[1] = 0  # an all-zero graph inside the batch
    got = totvar_loss(s.to(_dev()), a.to(_dev()), batch_reduction="sum")
    _check_value(name, got, R.totvar_terms(a, s).sum(), R.totvar_terms(a.double(), s.double()).sum())
    if name == "one_percent":
        per = totvar_loss(s[1:2].to(_dev()), a[1:2].to(_dev()))
        assert float(per) == 0.0


def test_totvar_graph_sizes_shorter_than_n():
    from tgp.utils.losses import acc_loss_terms
    a, s = _dense_batch(3, 150, 20, 0.1, 43, weighted=True)
    sizes = torch.tensor([150, 77, 0])
    keep = torch.arange(150).unsqueeze(0) < sizes.unsqueeze(1)
    a = a * keep.unsqueeze(1) * keep.unsqueeze(2)
    s = s * keep.unsqueeze(-1)
    dev = _dev()
    with_sizes = acc_loss_terms(a.to(dev), s.to(dev), 20, keep.to(dev), sizes.to(dev))
    without = acc_loss_terms(a.to(dev), s.to(dev), 20, keep.to(dev), None)
    assert torch.equal(with_sizes, without)  # (the skipped rows and columns are zero: the same sums in the same order)
    want = R.totvar_terms(a.double(), s.double())
    for b in range(2):
        _check_value(f"sizes[{b}]", with_sizes[0, b], R.totvar_terms(a, s)[b], want[b])
    assert float(with_sizes[0, 2]) == 0.0 and float(with_sizes[1, 2]) == 0.0


def test_totvar_dense_and_edge_forms_agree():
    """An unweighted graph without zero-weight edges: the nonzero entries are the edges, so the two forms state one
    number; both against the float64 restatement."""
    from tgp.utils.losses import sparse_totvar_loss, totvar_loss
    x, ei, _, batch = _graphs([300, 180, 257], 4, 6.0, 45, False)
    g = torch.Generator().manual_seed(46)
    sf = torch.softmax(torch.randn(x.size(0), 16, generator=g), -1)
    _, a, mask = R.O.dense_preprocessing(x, ei, torch.ones(ei.size(1)), batch, True)
    sd = torch.zeros(3, a.size(1), 16)
    sd[mask] = sf
    dev = _dev()
    dense = totvar_loss(sd.to(dev), a.to(dev))
    edge = sparse_totvar_loss(ei.to(dev), sf.to(dev), None, batch.to(dev))
    f64 = R.sparse_totvar_terms(ei, sf.double(), None, batch, 3).mean()
    f32 = R.sparse_totvar_terms(ei, sf, None, batch, 3).mean()
    _check_value("dense", dense, f32, f64)
    _check_value("edge", edge, f32, f64)
    bound, _ = _bound(f32, f64)
    assert abs(float(dense) - float(edge)) <= 2 * bound * abs(float(f64))


@pytest.mark.parametrize("adj_transpose", [True, False])
def test_totvar_is_invariant_to_adj_transpose(adj_transpose):
    x, ei, ew, batch = _graphs([90, 60, 120], 8, 5.0, 47, True, directed=True)
    ws, bs = _linears([8, 6], 48)
    case = _route_case("acc", dict(in_channels=8, k=6, adj_transpose=adj_transpose),
                       dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), ws, bs)
    out = _run(case)
    other = _run(dict(case, cfg=dict(case["cfg"], adj_transpose=not adj_transpose)))
    with torch.no_grad():
        l64, _, _ = R.pool_losses(case, torch.float64)
        l32, _, _ = R.pool_losses(case, torch.float32)
    for o in (out, other):
        _check_value("tv", o.loss["total_variation_loss"], l32["total_variation_loss"], l64["total_variation_loss"])


# ------------------------------------------------------------------------------------------------------------ routes
def _route_case(alias, cfg, inputs, weights, biases):
    params = {}
    for i, (w, b) in enumerate(zip(weights, biases)):
        params[f"selector.mlp.lins.{i}.weight"], params[f"selector.mlp.lins.{i}.bias"] = w, b
    return {"alias": alias, "cfg": cfg, "inputs": inputs, "params": params}


def _run(case, cls=None, train=False):
    dev = _dev()
    pooler = _pooler(case["alias"], case["cfg"], cls).to(dev)
    pooler.load_state_dict(case["params"])
    if train:
        return _call(pooler.train(), case["inputs"], dev)
    with torch.no_grad():
        return _call(pooler.eval(), case["inputs"], dev)


def _max_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def _check_route(case, out=None):
    out = _run(case) if out is None else out
    with torch.no_grad():
        l64, s64, p64 = R.pool_losses(case, torch.float64, device=_dev())
        l32, s32, p32 = R.pool_losses(case, torch.float32, device=_dev())
    for name, got, a32, a64 in (("s", out.so.s, s32, s64), ("x_pool", out.x, p32["x_pool"], p64["x_pool"]),
                                ("adj_pool", out.edge_index, p32["adj_pool"], p64["adj_pool"])):
        e32 = _max_rel(a32.reshape(a64.shape), a64)
        err = _max_rel(got.reshape(a64.shape), a64)
        print(f"{name}: e_kernel {err:.2e} e_oracle32 {e32:.2e}")
        assert err <= max(FACTOR * e32, 1e-5), (name, err, e32)
    for k in R.LOSSES:
        assert out.loss[k].dtype == torch.float32
        _check_value(k, out.loss[k], l32[k], l64[k])
    return out


def _sparse_case(alias, sizes, f, k, seed, deg=4.0, weighted=True, directed=False, **cfg):
    x, ei, ew, batch = _graphs(sizes, f, deg, seed, weighted, directed=directed)
    ws, bs = _linears([f, k], seed + 1)
    return _route_case(alias, dict(in_channels=f, k=k, **cfg), dict(x=x, edge_index=ei, edge_weight=ew, batch=batch),
                       ws, bs)


class _Spy:
    """Counts the calls of attributes of modules / classes and keeps what a ``note`` callable makes of each call."""

    def __init__(self, monkeypatch):
        self.mp, self.calls = monkeypatch, {}

    def on(self, owner, name, note=lambda a, kw, r: True):
        orig = getattr(owner, name)
        log = self.calls.setdefault(name, [])

        def spy(*a, **kw):
            r = orig(*a, **kw)
            log.append(note(a, kw, r))
            return r
        self.mp.setattr(owner, name, spy)
        return log


def _loss_spies(spy):
    from tgp import kernels as K
    return (spy.on(K, "acc_tv_dense", lambda a, kw, r: tuple(a[0].shape)),
            spy.on(K, "acc_tv_edge"),
            spy.on(K, "acc_quantile", lambda a, kw, r: ("flat" if kw.get("ptr") is not None else "dense", r[-1])))


def test_route_small_padded_batch(monkeypatch):
    """Dense padded inputs of small graphs (B >= 64, N <= 64, K and F <= 32): the one-launch Select + Reduce + Connect
    runs unchanged (no raw, no terms), the loss kernels run behind it on its S; the counting select."""
    from tgp import kernels as K
    spy = _Spy(monkeypatch)
    select = spy.on(K, "dense_pool_select", lambda a, kw, r: (kw.get("want_raw"), kw.get("mincut_terms")))
    tv, edge, quant = _loss_spies(spy)
    g = torch.Generator().manual_seed(5)
    B, N, F, Kc = 96, 24, 8, 6
    assert K.dense_pool_is_small(B, N, Kc, F)
    a = (torch.rand(B, N, N, generator=g) < 0.2).float() * (torch.rand(B, N, N, generator=g) + 0.1)
    mask = torch.arange(N).unsqueeze(0) < torch.randint(10, N + 1, (B, 1), generator=g)
    x = torch.randn(B, N, F, generator=g) * mask.unsqueeze(-1)
    ws, bs = _linears([F, Kc], 6)
    _check_route(_route_case("acc", dict(in_channels=F, k=Kc), dict(x=x, adj=a * mask.unsqueeze(1) * mask.unsqueeze(2),
                                                                    mask=mask), ws, bs))
    assert select == [(False, False)] and tv == [(B, N, N)] and edge == [] and quant == [("dense", "count")]


def test_route_small_sparse_batch_is_densified(monkeypatch):
    """A sorted batch of small graphs as PyG hands it over: ACC declines the one-launch sparse kernel (its total
    variation walks the dense adjacency) and the rows route; the batch is densified and takes the small padded route."""
    from tgp import kernels as K
    from tgp.poolers import _DenseMLPPooling
    spy = _Spy(monkeypatch)
    sparse = spy.on(_DenseMLPPooling, "_select_reduce_connect_sparse", lambda a, kw, r: r is not None)
    rows = spy.on(_DenseMLPPooling, "_unbatched_fused", lambda a, kw, r: r is not None)
    select = spy.on(K, "dense_pool_select", lambda a, kw, r: (kw.get("want_raw"), kw.get("mincut_terms")))
    native_sparse = spy.on(K, "dense_pool_select_sparse")
    tv, edge, quant = _loss_spies(spy)
    g = torch.Generator().manual_seed(7)
    sizes = torch.randint(20, 61, (256,), generator=g).tolist()
    _check_route(_sparse_case("acc", sizes, 32, 20, 8, directed=True))
    assert sparse == [False] and rows == [False] and native_sparse == []
    assert select == [(False, False)] and len(tv) == 1 and edge == [] and quant == [("dense", "count")]


def test_route_c2_dense_batch(monkeypatch):
    """B=32, N=1024, K=128, F=64 padded dense inputs: the operator route (Reduce + Connect, then the loss kernels on the
    dense adjacency); the radix select.  Also the C2 scale case."""
    from tgp import kernels as K
    spy = _Spy(monkeypatch)
    select = spy.on(K, "dense_pool_select")
    tv, edge, quant = _loss_spies(spy)
    g = torch.Generator().manual_seed(9)
    B, N, F, Kc = 32, 1024, 64, 128
    a = (torch.rand(B, N, N, generator=g) < 0.01).float()
    a = ((a + a.transpose(1, 2)) > 0).float()
    x = torch.randn(B, N, F, generator=g)
    ws, bs = _linears([F, Kc], 10)
    _check_route(_route_case("acc", dict(in_channels=F, k=Kc), dict(x=x, adj=a), ws, bs))
    assert select == [] and tv == [(B, N, N)] and edge == [] and quant == [("dense", "radix")]


def test_route_large_sparse_batch_declines_rows_route(monkeypatch):
    """Large sparse graphs: the rows route declines ACC, the batch is densified and takes the operator route."""
    from tgp import kernels as K
    from tgp.poolers import _DenseMLPPooling
    spy = _Spy(monkeypatch)
    rows = spy.on(_DenseMLPPooling, "_unbatched_fused", lambda a, kw, r: r is not None)
    select = spy.on(K, "dense_pool_select")
    tv, edge, quant = _loss_spies(spy)
    _check_route(_sparse_case("acc", [700, 512, 650, 600], 32, 32, 12, deg=6.0))
    assert rows == [False] and select == [] and tv == [(4, 700, 700)] and quant == [("dense", "radix")]


def test_route_unbatched(monkeypatch):
    """The unbatched pooler: the operator path with the edge-form total variation and the select on the flat layout."""
    from tgp.poolers import _DenseMLPPooling
    spy = _Spy(monkeypatch)
    rows = spy.on(_DenseMLPPooling, "_unbatched_fused", lambda a, kw, r: r is not None)
    tv, edge, quant = _loss_spies(spy)
    _check_route(_sparse_case("acc_u", [200, 256, 180], 16, 32, 14))
    assert rows == [False] and tv == [] and edge == [True] and quant == [("flat", "radix")]
    _check_route(_sparse_case("acc_u", [90, 60, 120], 8, 8, 16, directed=True))
    assert quant[-1] == ("flat", "count")


TRAIN_CASES = [
    ("small_batch_64", "acc", [10 + (i * 7) % 11 for i in range(64)], 5, 4),
    ("medium_batched", "acc", [200, 256, 180], 16, 32),
    ("large_batched", "acc", [700, 512], 32, 32),
    ("medium_unbatched", "acc_u", [200, 256, 180], 16, 32),
]


@pytest.mark.parametrize("name,alias,sizes,f,k", TRAIN_CASES, ids=[c[0] for c in TRAIN_CASES])
def test_route_training_is_the_operator_route(name, alias, sizes, f, k):
    """Training: _ACCTermsFn on the operator route; none of the one-node training functions takes ACC."""
    case = _sparse_case(alias, sizes, f, k, 30)
    out = _run(case, train=True)
    names = _graph_names(*(v.grad_fn for v in out.loss.values()), out.x.grad_fn)
    assert "_ACCTermsFnBackward" in names, names
    assert not set(ONE_NODE) & set(names), names


def test_other_dense_poolers_keep_their_routes(monkeypatch):
    """The predicate that names the loss-only kinds changes nothing for MinCut, DiffPool and DMoN, on the shapes whose
    one-node functions tests/test_gpu_grad_paths.py pins: a small sorted sparse batch takes the one-launch sparse kernel
    in inference for all three and _SelectPoolSparseFn in training for MinCut and DiffPool; larger graphs train through
    _PoolLargeFn (densifying route) or _PoolUnbatchedFn (rows route, unbatched poolers) for MinCut and DiffPool.  DMoN
    and ACC decline every one-node function."""
    import tgp.poolers as P
    from test_gpu_grad_paths import _small_sizes
    spy = _Spy(monkeypatch)
    sparse = spy.on(P._DenseMLPPooling, "_select_reduce_connect_sparse", lambda a, kw, r: r is not None)

    def nodes(case, cls, alias="acc"):
        out = _run(dict(case, alias=alias), cls, train=True)
        names = _graph_names(*(v.grad_fn for v in out.loss.values()), out.x.grad_fn, out.edge_index.grad_fn)
        return {n for n in ONE_NODE if n in names}

    others = ((P.MinCutPooling, True), (P.DiffPool, True), (P.DMoNPooling, False), (P.AsymCheegerCutPooling, False))
    small = {P.DiffPool: _sparse_case("acc", _small_sizes(602), 8, 13, 602)}
    for cls, one_node in others:
        case = small.get(cls, _sparse_case("acc", _small_sizes(601), 16, 7, 601))
        del sparse[:]
        _run(case, cls)
        assert sparse == [cls is not P.AsymCheegerCutPooling], cls.__name__
        assert nodes(case, cls) == ({"_SelectPoolSparseFnBackward"} if one_node else set()), cls.__name__
    monkeypatch.setattr(P, "_ROWS_ROUTE_DENSITY", 0.0)  # (the densifying route)
    for cls, one_node in others:
        case = _sparse_case("acc", [130, 97, 160], 24, 40, 340 if cls is not P.DiffPool else 440)
        assert nodes(case, cls) == ({"_PoolLargeFnBackward"} if one_node else set()), cls.__name__
    monkeypatch.setattr(P, "_ROWS_ROUTE_DENSITY", 2.0)  # (the rows route)
    for cls, one_node in others:
        if cls is P.DiffPool:
            case, alias = _sparse_case("acc_u", [130, 97, 160], 24, 40, 506, weighted=False), "acc_u"
        else:
            case, alias = _sparse_case("acc", [260, 199], 16, 72, 503, weighted=False), "acc"
        assert nodes(case, cls, alias) == ({"_PoolUnbatchedFnBackward"} if one_node else set()), cls.__name__


# --------------------------------------------------------------------------------------------------------- gradients
GRAD_CASES = [
    ("small_batched", "acc", [9, 6, 12], 5, 4),
    ("medium_batched", "acc", [200, 256, 180], 16, 32),
    ("small_unbatched", "acc_u", [9, 6, 12], 5, 4),
    ("medium_unbatched", "acc_u", [200, 256, 180], 16, 32),
    ("directed_batched", "acc", [40, 30, 50], 8, 8),
    ("directed_unbatched", "acc_u", [40, 30, 50], 8, 8),
    ("small_batch_64", "acc", [10 + (i * 7) % 11 for i in range(64)], 5, 4),
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
        losses, _, _ = R.pool_losses(case, dtype, "cpu", ws, bs, x)
        leaves = {"x": x}
        leaves.update(dict(zip(pnames, [t for pair in zip(ws, bs) for t in pair])))
        return losses, leaves
    return kernel, oracle, names


def _report(name, kernel, oracle, leaves):
    report = []
    fails = grad_path_errors(name, kernel, oracle, leaves, report=report)
    for path, leaf, e_k, e_32 in report:
        print(f"{name} | {path} | {leaf} | e_kernel {e_k:.2e} | e_oracle32 {e_32:.2e} | bound "
              f"{max(FACTOR * e_32, FLOOR):.2e} (cap {CAP:g})")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name,alias,sizes,f,k", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_gradient_paths_through_the_pooler(name, alias, sizes, f, k):
    kernel, oracle, leaves = _grad_runs(alias, sizes, f, k, 30, directed=name.startswith("directed"))
    _report(name, kernel, oracle, leaves)


@pytest.mark.parametrize("form,width", [("dense", 12), ("dense_mask", 12), ("flat", 12), ("flat_nobatch", 12),
                                        ("dense_mask", 300), ("flat", 300)])
def test_gradient_paths_through_the_functions(form, width):
    """Each of the four functions alone, S the leaf.  width = 300: more than 256 columns, the second column block of
    the two total-variation backward kernels."""
    from tgp.utils import losses as L
    x, ei, ew, batch = _graphs([150, 90, 201], 4, 5.0, 51, True, directed=True)
    g = torch.Generator().manual_seed(52)
    logits = torch.randn(x.size(0), width, generator=g)
    _, a, mask = R.O.dense_preprocessing(x, ei, ew, batch, False)
    k = width

    def leaf(dtype, dev):
        sf = torch.softmax(logits.to(dtype), -1).to(dev).requires_grad_(True)
        if form.startswith("flat"):
            return sf, sf
        sd = torch.zeros(3, a.size(1), width, dtype=dtype, device=dev)
        return sf, sd.masked_scatter(mask.to(dev).unsqueeze(-1), sf)

    def kernel():
        dev = _dev()
        sf, s = leaf(torch.float32, dev)
        if form == "dense":
            out = {"tv": L.totvar_loss(s, a.to(dev)), "bal": L.asym_norm_loss(s, k)}
        elif form == "dense_mask":
            out = {"tv": L.totvar_loss(s, a.to(dev), "sum"), "bal": L.asym_norm_loss(s, k, mask.to(dev), "sum")}
        elif form == "flat":
            out = {"tv": L.sparse_totvar_loss(ei.to(dev), s, ew.to(dev), batch.to(dev)),
                   "bal": L.unbatched_asym_norm_loss(s, k, batch.to(dev))}
        else:
            out = {"tv": L.sparse_totvar_loss(ei.to(dev), s, None), "bal": L.unbatched_asym_norm_loss(s, k)}
        return out, {"S": sf}

    def oracle(dtype):
        sf, s = leaf(dtype, "cpu")
        zeros = torch.zeros_like(batch)
        if form == "dense":
            out = {"tv": R.totvar_terms(a.to(dtype), s).mean(), "bal": R.asym_terms(s, k).mean()}
        elif form == "dense_mask":
            out = {"tv": R.totvar_terms(a.to(dtype), s).sum(), "bal": R.asym_terms(s, k, mask).sum()}
        elif form == "flat":
            out = {"tv": R.sparse_totvar_terms(ei, s, ew.to(dtype), batch, 3).mean(),
                   "bal": R.unbatched_asym_terms(s, k, batch, 3).mean()}
        else:
            out = {"tv": R.sparse_totvar_terms(ei, s, None, zeros, 1).mean(),
                   "bal": R.unbatched_asym_terms(s, k, zeros, 1).mean()}
        return out, {"S": sf}
    if form == "dense":  # (without a mask the padded zero rows tie at 0: keep the rows every graph has)
        n = int(mask.sum(1).min())
        a, mask = a[:, :n, :n].contiguous(), mask[:, :n]
        keep = torch.cat([torch.arange(o, o + n) for o in (0, 150, 240)])
        logits = logits[keep]
    _report(f"{form}-{width}", kernel, oracle, ["S"])


def test_composed_forms_take_what_the_kernels_do_not(monkeypatch):
    """An adjacency or edge weights that require grad, and an unsorted batch vector, take the composed torch forms (no
    loss kernel is launched); the values agree with the restatement and the adjacency / the weights get a gradient."""
    from tgp.utils import losses as L
    spy = _Spy(monkeypatch)
    tv, edge, quant = _loss_spies(spy)
    dev = _dev()
    a, s = _dense_batch(2, 60, 8, 0.2, 81, weighted=True)
    ad = a.to(dev).requires_grad_(True)
    got = L.totvar_loss(s.to(dev), ad)
    got.backward()
    assert tv == [] and ad.grad is not None and float(ad.grad.abs().sum()) > 0
    torch.testing.assert_close(got.cpu().double(), R.totvar_terms(a.double(), s.double()).mean(), rtol=1e-5, atol=1e-5)
    x, ei, ew, batch = _graphs([50, 70, 40], 4, 5.0, 82, True, directed=True)
    sf = torch.softmax(torch.randn(x.size(0), 8, generator=torch.Generator().manual_seed(83)), -1)
    wd = ew.to(dev).requires_grad_(True)
    got = L.sparse_totvar_loss(ei.to(dev), sf.to(dev), wd, batch.to(dev))
    got.backward()
    assert edge == [] and wd.grad is not None and float(wd.grad.abs().sum()) > 0
    want_tv = R.sparse_totvar_terms(ei, sf.double(), ew.double(), batch, 3).mean()
    torch.testing.assert_close(got.cpu().double(), want_tv, rtol=1e-5, atol=1e-5)
    assert L.acc_sparse_loss_terms(ei.to(dev), wd, sf.to(dev), 8, batch.to(dev)) is None
    # an unsorted batch vector: the nodes permuted, the edges relabelled
    perm = torch.randperm(x.size(0), generator=torch.Generator().manual_seed(84))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(x.size(0))
    bp, sp, eip = batch[perm].to(dev), sf[perm].to(dev), inv[ei].to(dev)
    assert not bool((bp[1:] >= bp[:-1]).all())
    got_tv = L.sparse_totvar_loss(eip, sp, ew.to(dev), bp)
    got_bal = L.unbatched_asym_norm_loss(sp, 8, bp)
    assert L.acc_sparse_loss_terms(eip, ew.to(dev), sp, 8, bp) is None
    assert tv == [] and edge == [] and quant == []
    torch.testing.assert_close(got_tv.cpu().double(), want_tv, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got_bal.cpu().double(), R.unbatched_asym_terms(sf.double(), 8, batch, 3).mean(),
                               rtol=1e-5, atol=1e-5)
    # the same operands without those properties do take the kernels
    L.sparse_totvar_loss(ei.to(dev), sf.to(dev), ew.to(dev), batch.to(dev))
    L.totvar_loss(s.to(dev), a.to(dev))
    assert len(tv) == 1 and len(edge) == 1


def test_unbatched_pooler_forms_both_losses_in_one_function(monkeypatch):
    """The unbatched pooler: one _ACCTermsFn call, one tail launch for both terms, coefficients applied."""
    from tgp import kernels as K
    spy = _Spy(monkeypatch)
    tails = spy.on(K, "acc_tail", lambda a, kw, r: tuple(float(c) for c in a[-1]))
    case = _sparse_case("acc_u", [200, 256, 180], 16, 32, 14, totvar_coeff=0.5, balance_coeff=2.0)
    _check_route(case)
    assert tails == [(0.5, 2.0)]
    out = _run(case, train=True)
    names = _graph_names(*(v.grad_fn for v in out.loss.values()))
    assert names.count("_ACCTermsFnBackward") == 1, names


def test_tied_quantile_gradient_goes_to_the_lowest_index():
    """Hand-built ties: every column holds its quantile value several times; the quantile's gradient lands on the
    lowest node index that holds it (tests/acc_restatement.quantile states the same rule), on both select routes and
    both layouts."""
    from tgp.utils.losses import asym_norm_loss, unbatched_asym_norm_loss
    dev = _dev()
    for n in (12, 200):
        g = torch.Generator().manual_seed(n)
        k = 4
        s = (torch.randint(0, 5, (2, n, 6), generator=g).float() / 4)
        want_node = torch.stack([R.quantile(s[b], k)[1] for b in range(2)])
        assert int((s == torch.stack([R.quantile(s[b], k)[0] for b in range(2)]).unsqueeze(1)).sum(1).max()) > 1
        s64 = s.double().requires_grad_(True)
        R.asym_terms(s64, k).sum().backward()
        sd = s.to(dev).requires_grad_(True)
        asym_norm_loss(sd, k, batch_reduction="sum").backward()
        torch.testing.assert_close(sd.grad.cpu().double(), s64.grad, rtol=1e-5, atol=1e-7)
        # the quantile node's entry is the only one in its column whose gradient differs from -rho'(d) / beta
        beta = n * (k - 1)
        d = s - s.gather(1, want_node.unsqueeze(1))
        plain = -torch.where(d >= 0, torch.tensor(float(k - 1)), torch.tensor(-1.0)) / beta
        differs = (sd.grad.cpu() - plain).abs() > 1e-6
        where = differs.to(torch.int64).argmax(1)
        assert torch.equal(differs.sum(1), torch.ones(2, 6, dtype=torch.long)) and torch.equal(where, want_node)
        sf = s.reshape(-1, 6).to(dev).requires_grad_(True)
        batch = torch.arange(2).repeat_interleave(n).to(dev)
        unbatched_asym_norm_loss(sf, k, batch, batch_reduction="sum").backward()
        assert torch.equal(sf.grad.view(2, n, 6), sd.grad)


# -------------------------------------------------------------------------------------------------------- determinism
def test_bitwise_determinism_c2_and_hub_graph():
    from tgp.utils.losses import acc_loss_terms, sparse_totvar_loss, unbatched_asym_norm_loss
    dev = _dev()
    a, s = _dense_batch(32, 1024, 128, 0.01, 61)
    a, s = a.to(dev), s.to(dev)

    def dense():
        leaf = s.clone().requires_grad_(True)
        out = acc_loss_terms(a, leaf, 128)
        out.sum().backward()
        return out.detach(), leaf.grad
    first, second = dense(), dense()
    for x, y in zip(first, second):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert float(first[0].abs().sum()) > 0 and float(first[1].abs().sum()) > 0
    # a hub graph: node 0 is joined to every other node in both directions (>= 100 000 edges), plus a ring
    n = 60000
    others = torch.arange(1, n)
    ei = torch.cat([torch.stack([torch.zeros_like(others), others]), torch.stack([others, torch.zeros_like(others)]),
                    torch.stack([others, others % (n - 1) + 1])], 1)
    ei = ei[:, torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(62))].to(dev)
    assert ei.size(1) >= 100000
    w = (torch.rand(ei.size(1), generator=torch.Generator().manual_seed(63)) + 0.1).to(dev)
    sf = torch.softmax(torch.randn(n, 16, generator=torch.Generator().manual_seed(64)), -1).to(dev)

    def hub():
        leaf = sf.clone().requires_grad_(True)
        out = sparse_totvar_loss(ei, leaf, w) + unbatched_asym_norm_loss(leaf, 16)
        out.backward()
        return out.detach(), leaf.grad
    first, second = hub(), hub()
    for x, y in zip(first, second):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    f64 = R.sparse_totvar_terms(ei.cpu(), sf.cpu().double(), w.cpu().double(), torch.zeros(n, dtype=torch.long), 1)[0]
    f32 = R.sparse_totvar_terms(ei.cpu(), sf.cpu(), w.cpu(), torch.zeros(n, dtype=torch.long), 1)[0]
    from tgp.utils.losses import sparse_totvar_loss as tv
    _check_value("hub", tv(ei, sf, w), f32, f64)


# -------------------------------------------------------------------------------------------------------------- scale
def test_scale_two_graphs_of_8192_nodes():
    """N = 8192, K = 512, 2 graphs: the kernels against the composed torch forms on the device (float64)."""
    from tgp.utils.losses import asym_norm_loss, totvar_loss
    dev = _dev()
    g = torch.Generator().manual_seed(71)
    B, N, K = 2, 8192, 512
    idx = torch.randint(0, N, (B, 2, 40000), generator=g)
    a = torch.zeros(B, N, N)
    for b in range(B):
        a[b, idx[b, 0], idx[b, 1]] = torch.rand(40000, generator=g) + 0.1
    s = torch.softmax(torch.randn(B, N, K, generator=g), -1)
    a, s = a.to(dev), s.to(dev)
    tv, bal = totvar_loss(s, a), asym_norm_loss(s, K)
    tv64, bal64 = totvar_loss(s.double(), a.double()), asym_norm_loss(s.double(), K)  # (the composed forms)
    assert tv64.dtype == torch.float64
    bi, ii, ji = a.nonzero(as_tuple=True)
    tv32 = torch.zeros(B, device=dev).index_add_(0, bi, a[bi, ii, ji] * (s[bi, ii] - s[bi, ji]).abs().sum(-1))
    tv32 = (tv32 / (2 * torch.bincount(bi, minlength=B).clamp(min=1))).mean()
    _check_value("totvar", tv, tv32, tv64)
    q = s.sort(dim=1, descending=True)[0][:, min(N // K, N - 1)]
    d = s - q.unsqueeze(1)
    beta = N * (K - 1)
    bal32 = ((beta - torch.where(d >= 0, (K - 1) * d, -d).sum((1, 2))) / beta).mean()
    # the balance loss is 1 - sum / beta: judged relative to 1, the larger of its two terms
    bound = max(FACTOR * abs(float(bal32) - float(bal64)), FLOOR)
    print(f"balance: kernel {float(bal):.9g} f64 {float(bal64):.9g} f32 {float(bal32):.9g} bound {bound:.2e}")
    assert abs(float(bal) - float(bal64)) <= bound
