"""Just Balance pooling on the GPU.

* Fixture parity: every pooler case of tests/golden/golden_jb_v1.pt (made by the reference, tests/golden/make_golden_jb.py)
  at the project's rtol = atol = 1e-5: S, x, the pooled adjacency or edges (indices exact), batch and the loss.
* The loss kernels and each route, forced by shape, against the float64 restatement (tests/jb_restatement.py) by maximum
  relative error.  The bound is ROUTE_REL = 1e-5, the project's fp32 tolerance, by test_gpu_dmon.py's derivation: fp32's
  unit roundoff (6e-8) times the longest reduction here (1024 rows) grown as its square root is 2e-6, and every sum runs
  over non-negative terms.  The loss is a sum of terms of one sign and is judged relative to itself (per graph for the
  kernels, the batch mean for the routes); tensors relative to their max-norm.
* Bit-reproducibility: the same call twice gives equal bits, forward and backward (no float atomics).
* Gradients of the loss, with tests/test_gpu_grad_paths.py's helper and constants, the restatement as the fp64 and fp32
  oracle.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jb_restatement as R  # noqa: E402
from test_gpu_golden import check_output, check_so  # noqa: E402
from test_gpu_grad_paths import CAP, FACTOR, FLOOR, _graph_names, _graphs, _linears, grad_path_errors  # noqa: E402
from test_jb_restatement import function_values  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = torch.load(os.path.join(HERE, "golden", "golden_jb_v1.pt"), weights_only=True)["cases"]
POOL = sorted(k for k, v in CASES.items() if v["kind"] == "pool")
ROUTE_REL = 1e-5
F64_REL = 1e-10
STRADDLE = [63, 64, 65, 129]  # rows around PART_ROWS = 64: one split exactly, one row into the second, three splits


def _dev():
    return torch.device("cuda:0")


def _pooler(alias, cfg):
    from tgp.poolers import JustBalancePooling
    return JustBalancePooling(**cfg, batched=(alias == "jb"))


def _call(pooler, inp, dev):
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    if "adj" in d:
        return pooler(x=d["x"], adj=d["adj"], mask=d.get("mask"))
    return pooler(x=d["x"], adj=d["edge_index"], edge_weight=d.get("edge_weight"), batch=d.get("batch"))


# ----------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", POOL)
def test_fixture_parity(name):
    c = CASES[name]
    pooler = _pooler(c["alias"], c["cfg"]).to(_dev()).eval()
    pooler.load_state_dict(c["params"])
    with torch.no_grad():
        out = _call(pooler, c["inputs"], _dev())
    check_so(out.so, c["expected"]["so"], name)
    check_output(out, c["expected"], name)
    assert list(out.loss) == ["balance_loss"]
    assert out.loss["balance_loss"].dim() == 0 and out.loss["balance_loss"].dtype == torch.float32


@pytest.mark.parametrize("name", ["jb_batched_default_w", "jb_batched_mlp2_u", "jb_batched_coeff05_w",
                                  "jb_unbatched_nonorm_w", "jb_dense_inputs_mask_dirty_x", "jb_u_single_graph"])
def test_fixture_parity_under_autograd(name):
    """Training takes the operator route (reduce_connect's differentiable form + the loss Function): same values."""
    c = CASES[name]
    pooler = _pooler(c["alias"], c["cfg"]).to(_dev())
    pooler.load_state_dict(c["params"])
    out = _call(pooler, c["inputs"], _dev())
    check_output(out, c["expected"], name + ".train")
    assert "_JBTermsFnBackward" in _graph_names(out.loss["balance_loss"].grad_fn)
    out.loss["balance_loss"].backward()
    g = pooler.selector.mlp.lins[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0


def test_public_loss_functions():
    from tgp.utils.losses import jb_loss_terms, just_balance_loss, unbatched_just_balance_loss
    for tag in ("f32", "f64"):
        c = CASES[f"jb_functions_{tag}"]
        i = {k: v.to(_dev()) for k, v in c["inputs"].items()}
        e = c["expected"]

        def dense(s, mask=None, normalize=True, num_nodes=None, num_supernodes=None):
            return jb_loss_terms(s, mask, None, None, normalize, num_nodes, num_supernodes)

        def flat(s, batch=None, normalize=True):
            return jb_loss_terms(s, batch=batch, normalize_loss=normalize)
        got = function_values(i, dense, flat)
        got["mask"] = just_balance_loss(i["s"], i["mask"])
        got["dirty_mask_sum"] = just_balance_loss(i["s_dirty"], i["mask"], batch_reduction="sum")
        got["nomask_n5_k6"] = just_balance_loss(i["s"], None, True, 5, 6)
        got["unbatched_sum"] = unbatched_just_balance_loss(i["s_flat"], i["batch"], batch_reduction="sum")
        got["unbatched_nobatch"] = unbatched_just_balance_loss(i["s_flat"])
        assert set(got) == set(e)
        for k, v in got.items():
            assert v.dtype == e[k].dtype, (tag, k)
            torch.testing.assert_close(v.cpu(), e[k], rtol=1e-5, atol=1e-5, msg=lambda m: f"{tag}.{k}: {m}")
        perm = torch.randperm(i["batch"].numel(), generator=torch.Generator().manual_seed(0)).to(_dev())
        v = unbatched_just_balance_loss(i["s_flat"][perm], i["batch"][perm])  # unsorted: the composed form
        torch.testing.assert_close(v.cpu(), e["unbatched"], rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------------- loss kernels
def _max_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def _per_graph_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(((a - b).abs() / b.abs()).max())


def _flat_batch(sizes, k, seed, zero_col=None):
    g = torch.Generator().manual_seed(seed)
    n = sum(sizes)
    s = torch.softmax(2 * torch.randn(n, k, generator=g), -1) if k > 1 else torch.rand(n, 1, generator=g)
    if zero_col is not None:
        s[:, zero_col] = 0.0
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return s, batch


def _pad(s, batch, sizes):
    n = max(sizes)
    out = torch.zeros(len(sizes), n, s.size(1), dtype=s.dtype)
    mask = torch.zeros(len(sizes), n, dtype=torch.bool)
    off = 0
    for b, c in enumerate(sizes):
        out[b, :c] = s[off:off + c]
        mask[b, :c] = True
        off += c
    return out, mask


def _check_terms(got, s_dev, want64, grad_of):
    """Per-graph values relative to themselves, dS (upstream: distinct per-graph weights) relative to its max-norm."""
    assert got.dtype == torch.float32
    e = _per_graph_rel(got, want64)
    up = torch.linspace(0.5, 1.5, got.numel())
    (gs,) = torch.autograd.grad(got, s_dev, up.to(got.device))
    e_g = _max_rel(gs, grad_of(up.double()))
    print(f"terms {e:.2e} dS {e_g:.2e}")
    assert e <= ROUTE_REL and e_g <= ROUTE_REL, (e, e_g)
    return gs


@pytest.mark.parametrize("k", [1, 3, 4, 70, 257, 260])
def test_kernels_flat_and_padded_rows_straddling_a_split(k):
    """Graphs of 63, 64, 65 and 129 rows (partial pass + tail), K below, at and beyond a row group's 64 lanes and a
    workgroup's 256 threads, not a multiple of 4 (element loads) and a multiple (16-byte loads; 260: more 16-byte units
    than a row group has lanes); a zero column."""
    from tgp.utils.losses import jb_loss_terms
    s, batch = _flat_batch(STRADDLE, k, 40 + k, zero_col=0 if k > 1 else None)
    s64 = s.double().requires_grad_(True)
    want = R.flat_terms(s64, batch)
    sd = s.to(_dev()).requires_grad_(True)
    got = jb_loss_terms(sd, batch=batch.to(_dev()))
    gs = _check_terms(got, sd, want, lambda up: torch.autograd.grad(want, s64, up, retain_graph=True)[0])
    if k > 1:
        assert bool((gs[:, 0] == 0).all())  # c_k = 0: coef stays finite, the gradient is 0
    # the same rows padded: with the mask (all N rows summed, n_b counted from the mask) and with graph sizes
    sp, mask = _pad(s, batch, STRADDLE)
    sp64 = sp.double().requires_grad_(True)
    want_p = R.dense_terms(sp64, mask)
    for sizes in (None, torch.tensor(STRADDLE)):
        spd = sp.to(_dev()).requires_grad_(True)
        got = jb_loss_terms(spd, mask.to(_dev()), None if sizes is None else sizes.to(_dev()))
        _check_terms(got, spd, want_p, lambda up: torch.autograd.grad(want_p, sp64, up, retain_graph=True)[0])
        assert _per_graph_rel(got, want) <= ROUTE_REL  # (and the padded and the un-padded forms agree)


def test_kernels_one_launch_small_graphs_and_variants(monkeypatch):
    """64 graphs of 10-20 nodes: every graph fits one split, so forward is ONE native call that needs no part buffer;
    normalize_loss=False, a scale, explicit num_nodes / num_supernodes, the sum reduction's dense upstream gradient."""
    from tgp import kernels as K
    from tgp.utils.losses import jb_loss_terms
    sizes = [10 + (i * 7) % 11 for i in range(64)]
    for k in (4, 20, 7):
        s, batch = _flat_batch(sizes, k, 60 + k)
        s64 = s.double().requires_grad_(True)
        want = R.flat_terms(s64, batch)
        sd = s.to(_dev()).requires_grad_(True)
        _check_terms(jb_loss_terms(sd, batch=batch.to(_dev())), sd, want,
                     lambda up: torch.autograd.grad(want, s64, up, retain_graph=True)[0])
        sp, mask = _pad(s, batch, sizes)
        got = jb_loss_terms(sp.to(_dev()), mask.to(_dev()), torch.tensor(sizes).to(_dev()))
        assert _per_graph_rel(got, want) <= ROUTE_REL
        got = jb_loss_terms(sp.to(_dev()), None, None, None, False, scale=0.5)
        assert _per_graph_rel(got, 0.5 * R.dense_terms(sp.double(), None, normalize=False)) <= ROUTE_REL
        got = jb_loss_terms(sp.to(_dev()), None, None, None, True, 13, 9)
        assert _per_graph_rel(got, R.dense_terms(sp.double(), None, True, 13, 9)) <= ROUTE_REL
    lib = K.N.lib()
    seen = []
    orig = lib.tgp_jb_terms_f32

    def spy(*a):
        seen.append(a[13])  # the part buffer
        return orig(*a)
    monkeypatch.setattr(lib, "tgp_jb_terms_f32", spy)
    K.jb_terms(sp.to(_dev()))
    K.jb_terms(torch.zeros(2, 65, 4, device=_dev()))
    assert seen[0] is None and seen[1] is not None  # one launch up to 64 rows, the partial pass beyond


def test_kernels_mask_with_holes_and_rows_that_are_not_zero():
    """The public padded form: a mask with holes in the middle of a graph and an S whose masked rows are NOT zero --
    every row of S counts, the mask only gives n_b; one graph without a real node gives -inf, as the composed form."""
    from tgp.utils.losses import just_balance_loss
    g = torch.Generator().manual_seed(77)
    for n, k in ((20, 5), (130, 8)):
        s = torch.softmax(torch.randn(5, n, k, generator=g), -1)
        mask = torch.rand(5, n, generator=g) < 0.7
        mask[0] = True
        mask[1, n // 2:] = False
        sd = s.to(_dev()).requires_grad_(True)
        s64 = s.double().requires_grad_(True)
        got = just_balance_loss(sd, mask.to(_dev()), batch_reduction="sum")
        want = R.dense_terms(s64, mask).sum()
        assert abs(float(got.detach()) - float(want.detach())) <= ROUTE_REL * abs(float(want.detach()))
        (gs,) = torch.autograd.grad(got, sd)
        assert _max_rel(gs, torch.autograd.grad(want, s64)[0]) <= ROUTE_REL
        mask[2] = False
        assert float(just_balance_loss(s.to(_dev()), mask.to(_dev()))) == float("-inf")
        assert float(R.dense_terms(s.double(), mask).mean()) == float("-inf")


@pytest.mark.parametrize("sizes,k", [(STRADDLE, 8), ([12, 20, 17], 4)])
def test_kernels_pointer_offset_by_four_bytes(sizes, k):
    """S a contiguous slice that starts 4 bytes into its buffer: K % 4 == 0 but the rows are not 16-byte aligned, so
    the element-load kernels run (forward and backward); same values as the aligned copy to the last bit or two."""
    from tgp.utils.losses import jb_loss_terms
    s, batch = _flat_batch(sizes, k, 90)
    buf = torch.zeros(s.numel() + 1, device=_dev())
    buf[1:] = s.reshape(-1).to(_dev())
    off = buf[1:].view(s.shape)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    off = off.requires_grad_(True)
    al = s.to(_dev()).requires_grad_(True)
    assert al.data_ptr() % 16 == 0
    bd = batch.to(_dev())
    want = R.flat_terms(s.double(), batch)
    got_off, got_al = jb_loss_terms(off, batch=bd), jb_loss_terms(al, batch=bd)
    assert _per_graph_rel(got_off, want) <= ROUTE_REL and _per_graph_rel(got_al, want) <= ROUTE_REL
    g_off, g_al = torch.autograd.grad(got_off.sum(), off)[0], torch.autograd.grad(got_al.sum(), al)[0]
    assert _max_rel(g_off, g_al) <= ROUTE_REL


def test_bit_reproducibility():
    from tgp.utils.losses import jb_loss_terms
    for sizes, k in ((STRADDLE, 70), ([10 + (i * 7) % 11 for i in range(64)], 20), ([700, 1024, 333], 128)):
        s, batch = _flat_batch(sizes, k, 101)
        runs = []
        for _ in range(2):
            sd = s.to(_dev()).requires_grad_(True)
            out = jb_loss_terms(sd, batch=batch.to(_dev()))
            (gs,) = torch.autograd.grad(out.mean(), sd)  # (a mean: the expanded-scalar upstream gradient)
            runs.append((out.detach().clone(), gs.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        sp, mask = _pad(s, batch, sizes)
        a = jb_loss_terms(sp.to(_dev()), mask.to(_dev()))
        b = jb_loss_terms(sp.to(_dev()), mask.to(_dev()))
        assert torch.equal(a, b)
        # inference's form of the same call: no coefficients, the batch mean from a launch of the same native call
        from tgp import kernels as K
        one = K.jb_terms(sp.to(_dev()), mask=mask.to(_dev()), want_coef=False, want_mean=True)
        two = K.jb_terms(sp.to(_dev()), mask=mask.to(_dev()), want_coef=False, want_mean=True)
        assert one[1] is None and torch.equal(one[0], a) and torch.equal(one[2], two[2]) and one[2].dim() == 0
        want = a.double().mean()
        assert abs(float(one[2]) - float(want)) <= ROUTE_REL * abs(float(want))


# ------------------------------------------------------------------------------------------------------------ routes
def _route_case(alias, cfg, inputs, weights, biases):
    params = {}
    for i, (w, b) in enumerate(zip(weights, biases)):
        params[f"selector.mlp.lins.{i}.weight"], params[f"selector.mlp.lins.{i}.bias"] = w, b
    return {"alias": alias, "cfg": cfg, "inputs": inputs, "params": params}


def _check_route(case, bound=ROUTE_REL, dtype=torch.float32):
    dev = _dev()
    pooler = _pooler(case["alias"], case["cfg"]).to(dev).to(dtype).eval()
    pooler.load_state_dict({k: v.to(dtype) for k, v in case["params"].items()})
    inp = {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
           for k, v in case["inputs"].items()}
    with torch.no_grad():
        out = _call(pooler, inp, dev)
        ref, s_ref, pooled = R.pool_losses(case, torch.float64, device=dev)
    assert out.loss["balance_loss"].dtype == dtype
    errs = {"s": _max_rel(out.so.s, s_ref.reshape(out.so.s.shape)), "x_pool": _max_rel(out.x, pooled["x_pool"]),
            "adj_pool": _max_rel(out.edge_index, pooled["adj_pool"]),
            "balance_loss": abs(float(out.loss["balance_loss"]) - float(ref["balance_loss"]))
            / abs(float(ref["balance_loss"]))}
    print(case.get("name", ""), {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= bound, (k, v, bound)
    return out


def _sparse_case(alias, sizes, f, k, seed, deg=4.0, weighted=True, **cfg):
    x, ei, ew, batch = _graphs(sizes, f, deg, seed, weighted)
    ws, bs = _linears([f, k], seed + 1)
    return _route_case(alias, dict(in_channels=f, k=k, **cfg), dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), ws, bs)


class _Spies:
    """Counts the calls that tell the routes apart: the loss kernel's layout, the densification, the rows route."""

    def __init__(self, monkeypatch):
        from tgp import kernels as K
        from tgp.poolers import _DenseMLPPooling
        self.jb, self.densified, self.rows, self.select, self.select_sparse = [], [], [], [], []
        o_jb, o_dense, o_rows = K.jb_terms, _DenseMLPPooling._ensure_batched_inputs, _DenseMLPPooling._unbatched_fused
        o_sel, o_sels = K.dense_pool_select, K.dense_pool_select_sparse

        def jb(s, *a, **kw):
            self.jb.append(("flat" if kw.get("ptr") is not None else "dense", tuple(s.shape),
                            kw.get("graph_sizes") is not None))
            return o_jb(s, *a, **kw)

        def dense(this, *a, **kw):
            r = o_dense(this, *a, **kw)
            self.densified.append(tuple(r[1].shape))
            return r

        def rows(this, *a, **kw):
            r = o_rows(this, *a, **kw)
            self.rows.append(r is not None and r.x_pool is not None)
            return r

        def sel(*a, **kw):
            self.select.append((kw.get("want_raw"), kw.get("mincut_terms")))
            return o_sel(*a, **kw)

        def sels(*a, **kw):
            self.select_sparse.append((kw.get("want_raw"), kw.get("mincut_terms"), bool(kw.get("want_dense"))))
            return o_sels(*a, **kw)
        monkeypatch.setattr(K, "jb_terms", jb)
        monkeypatch.setattr(_DenseMLPPooling, "_ensure_batched_inputs", dense)
        monkeypatch.setattr(_DenseMLPPooling, "_unbatched_fused", rows)
        monkeypatch.setattr(K, "dense_pool_select", sel)
        monkeypatch.setattr(K, "dense_pool_select_sparse", sels)


def test_route_small_padded_batch(monkeypatch):
    """Dense padded inputs of small graphs: the one-launch Select + Reduce + Connect without raw and without terms, then
    the one-launch loss kernel on its S."""
    from tgp import kernels as K
    spies = _Spies(monkeypatch)
    g = torch.Generator().manual_seed(5)
    B, N, F, Kc = 96, 24, 8, 6
    assert K.dense_pool_is_small(B, N, Kc, F)
    a = (torch.rand(B, N, N, generator=g) < 0.2).float() * (torch.rand(B, N, N, generator=g) + 0.1)
    mask = torch.arange(N).unsqueeze(0) < torch.randint(10, N + 1, (B, 1), generator=g)
    x = torch.randn(B, N, F, generator=g) * mask.unsqueeze(-1)
    ws, bs = _linears([F, Kc], 6)
    _check_route(_route_case("jb", dict(in_channels=F, k=Kc), dict(x=x, adj=a * mask.unsqueeze(1) * mask.unsqueeze(2),
                                                                    mask=mask), ws, bs))
    assert spies.select == [(False, False)] and spies.jb == [("dense", (B, N, Kc), False)]


@pytest.mark.parametrize("cfg", [dict(), dict(adj_transpose=False, normalize_loss=False, loss_coeff=0.25)])
def test_route_small_sparse_batch(cfg, monkeypatch):
    """A sorted batch of small graphs as PyG hands it over: the one-launch sparse kernel without raw, the loss kernel on
    its S with the graph sizes; nothing is densified."""
    spies = _Spies(monkeypatch)
    g = torch.Generator().manual_seed(7)
    sizes = torch.randint(20, 61, (256,), generator=g).tolist()
    _check_route(_sparse_case("jb", sizes, 32, 20, 8, **cfg))
    assert spies.select_sparse == [(False, False, False)] and spies.densified == []
    assert spies.jb == [("dense", (256, max(sizes), 20), True)]


def test_route_large_dense_batch(monkeypatch):
    """Padded dense inputs beyond the one-wave kernels, a mask with graphs of 63, 64, 65 and 129 nodes: the operator
    route (reduce_connect without raw), the partial pass and the tail over all N rows."""
    spies = _Spies(monkeypatch)
    g = torch.Generator().manual_seed(9)
    B, N, F, Kc = 4, 129, 16, 12
    mask = torch.arange(N).unsqueeze(0) < torch.tensor(STRADDLE).unsqueeze(1)
    a = (torch.rand(B, N, N, generator=g) < 0.05).float()
    a = ((a + a.transpose(1, 2)) > 0).float() * mask.unsqueeze(1) * mask.unsqueeze(2)
    x = torch.randn(B, N, F, generator=g) * mask.unsqueeze(-1)
    ws, bs = _linears([F, Kc], 10)
    _check_route(_route_case("jb", dict(in_channels=F, k=Kc), dict(x=x, adj=a, mask=mask), ws, bs))
    assert spies.select == [] and spies.jb == [("dense", (B, N, Kc), False)]


def test_route_rows(monkeypatch):
    """[200, 256, 180] nodes, K = 32, four neighbours per node: too large for the one-launch kernels and sparse enough
    for the un-padded rows route -- SpMM, S^T [A S | X], the flat loss kernel on S with ptr; no [B,N,N] tensor."""
    spies = _Spies(monkeypatch)
    out = _check_route(_sparse_case("jb", [200, 256, 180], 16, 32, 14))
    assert spies.rows == [True] and spies.densified == [] and spies.select_sparse == []
    assert spies.jb == [("flat", (636, 32), False)]
    assert tuple(out.so.s.shape) == (3, 256, 32)


def test_route_rows_declined_takes_the_densifying_route(monkeypatch):
    """The same batch with the rows route switched off: densified, operator route, same values."""
    import tgp.poolers as P
    monkeypatch.setattr(P, "_ROWS_ROUTE", False)
    spies = _Spies(monkeypatch)
    _check_route(_sparse_case("jb", [200, 256, 180], 16, 32, 14))
    assert spies.rows == [False] and spies.densified == [(3, 256, 256)]
    assert spies.jb == [("dense", (3, 256, 32), True)]


def test_route_unbatched(monkeypatch):
    """batched=False: the operator path, compute_sparse_loss on the flat layout."""
    spies = _Spies(monkeypatch)
    _check_route(_sparse_case("jb_u", [200, 256, 180], 16, 32, 14))
    _check_route(_sparse_case("jb_u", STRADDLE, 8, 6, 15, normalize_loss=False))
    assert spies.densified == [] and [j[0] for j in spies.jb] == ["flat", "flat"]


def test_route_training_declines_the_one_node_paths(monkeypatch):
    """Under autograd every shape takes the operator route: the rows route and the one-launch sparse kernel decline."""
    spies = _Spies(monkeypatch)
    dev = _dev()
    for sizes, f, k in (([200, 256, 180], 16, 32), ([10 + (i * 7) % 11 for i in range(64)], 5, 4)):
        case = _sparse_case("jb", sizes, f, k, 30)
        pooler = _pooler("jb", case["cfg"]).to(dev)
        pooler.load_state_dict(case["params"])
        out = _call(pooler, case["inputs"], dev)
        names = _graph_names(out.loss["balance_loss"].grad_fn)
        assert "_JBTermsFnBackward" in names, names
        assert not any(n.startswith(("_PoolUnbatchedFn", "_PoolLargeFn", "_SelectPool")) for n in names), names
    assert spies.rows == [False, False] and spies.select_sparse == [] and len(spies.densified) == 2


def test_route_float64():
    for alias in ("jb", "jb_u"):
        _check_route(_sparse_case(alias, [90, 60, 120], 8, 8, 18), bound=F64_REL, dtype=torch.float64)


# --------------------------------------------------------------------------------------------------------- gradients
GRAD_CASES = [
    ("small_batched", "jb", [9, 6, 12], 5, 4),
    ("medium_batched", "jb", [200, 256, 180], 16, 32),
    ("small_unbatched", "jb_u", [9, 6, 12], 5, 4),
    ("medium_unbatched", "jb_u", [200, 256, 180], 16, 32),
    ("small_batch_64", "jb", [10 + (i * 7) % 11 for i in range(64)], 5, 4),
]


def _grad_runs(alias, sizes, f, k, seed):
    case = _sparse_case(alias, sizes, f, k, seed)
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


@pytest.mark.parametrize("name,alias,sizes,f,k", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_gradient_paths(name, alias, sizes, f, k):
    kernel, oracle, leaves = _grad_runs(alias, sizes, f, k, 30)
    report = []
    fails = grad_path_errors(name, kernel, oracle, leaves, report=report)
    for path, leaf, e_k, e_32 in report:
        print(f"{name} | {path} | {leaf} | e_kernel {e_k:.2e} | e_oracle32 {e_32:.2e} | bound "
              f"{max(FACTOR * e_32, FLOOR):.2e} (cap {CAP:g})")
    assert report and not fails, "\n".join(fails)
