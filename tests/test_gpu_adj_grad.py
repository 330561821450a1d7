"""The dense poolers' native adjacency gradient (csrc/dense_adj_grad.hip): a dense float32 adjacency [B,N,N] that is
handed to DiffPool / MinCut and requires a gradient -- what the second level of a stacked model receives -- stays on the
one-node training routes and gets dA from a launch behind the node's backward.

* route: which route method answers, how many pooling nodes the autograd graph holds, and the module flag that turns the
  gate off (the assertions that fail without the feature);
* gradients: every differentiable output is sent back alone (``grad_path_errors`` of tests/test_gpu_grad_paths.py, its
  rule and constants unchanged) with ``adj`` among the leaves;
* the two kernels alone against the float64 restatement (tests/adj_grad_restatement.py), bad arguments, bitwise
  repeatability, peak memory of the backward, the native calls when A is data, and a two-level model.

Shapes: the smallest that reach each code path -- the one-wave kernel's minimum of 64 graphs with N in {12, 40, 64} and
K in {3, 12}; the tiled kernel with N in {80, 130} (one and two 128-row tiles, all of them edge tiles) and K in {3, 33}
(one and two k-steps, K no multiple of 4), plus N = 260 / K = 32 for the kernels alone (interior tiles: the 16-byte
epilogue and operand loads)."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adj_grad_restatement as R  # noqa: E402
from test_gpu_dense_pooler_routes import ROUTES, _Recorder  # noqa: E402
from test_gpu_grad_paths import CAP, FACTOR, FLOOR, _graph_names, _rel, check_grad_paths  # noqa: E402

POOL_NODES = ("_PoolLargeFn", "_SelectPoolSmallFn", "_DensePoolSmallFn")


def _dev():
    return torch.device("cuda:0")


def _ragged(B, N):
    """Real nodes per graph: all of N, one node, and sizes in between."""
    sizes = [1 + (7 * i) % N for i in range(B)]
    sizes[0], sizes[1] = N, 1
    return sizes


class AdjCase:
    """One DiffPool / MinCut call in training on a dense adjacency that is a leaf."""

    def __init__(self, alias, B, N, K, F, *, seed, masked, hidden=None, adj_transpose=True, normalize_loss=False,
                 route=None, node=None):
        self.alias, self.hidden, self.route, self.node = alias, hidden, route, node
        self.cfg = dict(adj_transpose=adj_transpose)
        if alias == "diff":
            self.cfg["normalize_loss"] = normalize_loss
        self.x, self.adj, self.mask, self.ws, self.bs = R.make_inputs(
            B, N, K, F, seed, sizes=_ragged(B, N) if masked else None, hidden=hidden)
        self.k, self.f = K, F
        self.name = "-".join([alias, f"B{B}", f"N{N}", f"K{K}", "masked" if masked else "unmasked",
                              "hidden" if hidden else "linear", "at" if adj_transpose else "noat"]
                             + (["norm"] if normalize_loss else []))
        self.leaves = ["x", "adj"] + [f"W{i}" for i in range(len(self.ws))] + [f"b{i}" for i in range(len(self.bs))]

    def oracle(self, dtype):
        outs, lv, _ = R.oracle_run(self.alias, self.x, self.adj, self.mask, self.ws, self.bs, dtype,
                                   hidden=bool(self.hidden), **self.cfg)
        return outs, lv

    def pooler(self):
        from tgp.poolers import get_pooler
        chans = self.f if not self.hidden else [self.f, self.hidden]
        pooler = get_pooler(self.alias, in_channels=chans, k=self.k, **({"act": "tanh"} if self.hidden else {}),
                            **self.cfg).to(_dev()).train()
        lins = pooler.selector.mlp.lins
        assert len(lins) == len(self.ws)
        with torch.no_grad():
            for lin, w, b in zip(lins, self.ws, self.bs):
                lin.weight.copy_(w)
                lin.bias.copy_(b)
        return pooler

    def run(self, adj_grad=True):
        """(outputs by path name, leaves by name, autograd node names) of the product."""
        dev = _dev()
        pooler = self.pooler()
        xg = self.x.to(dev).requires_grad_(True)
        ag = self.adj.to(dev).requires_grad_(adj_grad)
        out = pooler(x=xg, adj=ag, mask=None if self.mask is None else self.mask.to(dev))
        outs = {"x": out.x, "adj": out.edge_index}
        for i, (n, v) in enumerate(out.loss.items()):
            outs[f"loss{i + 1}:{n}"] = v
        lv = {"x": xg, "adj": ag}
        for i, lin in enumerate(pooler.selector.mlp.lins):
            lv[f"W{i}"], lv[f"b{i}"] = lin.weight, lin.bias
        return outs, lv, _graph_names(*(v.grad_fn for v in outs.values()))

    def kernel(self):
        return self.run()[:2]


_TRAIN, _LARGE = "_select_reduce_connect_train", "_select_reduce_connect_large"
# the one-wave route: 64 graphs (the kernel's minimum), F = 4.  A hidden layer hands S to functions._DensePoolSmallFn
# (no route method answers: Reduce + Connect are the fused node).  DiffPool with a mask keeps its two losses on the
# operator route, as before (their normalisation needs the node count on the host): the pooling node is the fused one.
SMALL = [
    AdjCase("mincut", 64, 12, 3, 4, seed=1201, masked=True, route=_TRAIN, node="_SelectPoolSmallFn"),
    AdjCase("mincut", 64, 40, 12, 4, seed=1202, masked=True, adj_transpose=False, route=_TRAIN, node="_SelectPoolSmallFn"),
    AdjCase("mincut", 64, 64, 12, 4, seed=1203, masked=False, hidden=6, adj_transpose=False, node="_DensePoolSmallFn"),
    AdjCase("mincut", 64, 64, 3, 4, seed=1204, masked=True, route=_TRAIN, node="_SelectPoolSmallFn"),
    AdjCase("diff", 64, 12, 12, 4, seed=1205, masked=False, route=_TRAIN, node="_SelectPoolSmallFn"),
    AdjCase("diff", 64, 40, 3, 4, seed=1206, masked=False, adj_transpose=False, normalize_loss=True, route=_TRAIN,
            node="_SelectPoolSmallFn"),
    AdjCase("diff", 64, 64, 12, 4, seed=1207, masked=False, hidden=6, normalize_loss=True, node="_DensePoolSmallFn"),
    AdjCase("diff", 64, 64, 3, 4, seed=1208, masked=True, adj_transpose=False, route=_TRAIN, node="_SelectPoolSmallFn"),
]
# the large route: B = 2, F = 5; 130 is no tile multiple, 33 no multiple of 4 and more than one k-step
LARGE = [
    AdjCase("mincut", 2, 80, 3, 5, seed=1301, masked=True, route=_LARGE, node="_PoolLargeFn"),
    AdjCase("mincut", 2, 130, 33, 5, seed=1302, masked=False, adj_transpose=False, route=_LARGE, node="_PoolLargeFn"),
    AdjCase("mincut", 2, 130, 3, 5, seed=1303, masked=True, hidden=7, adj_transpose=False, route=_LARGE, node="_PoolLargeFn"),
    AdjCase("mincut", 2, 80, 33, 5, seed=1304, masked=False, hidden=7, route=_LARGE, node="_PoolLargeFn"),
    AdjCase("diff", 2, 80, 3, 5, seed=1305, masked=False, normalize_loss=True, route=_LARGE, node="_PoolLargeFn"),
    AdjCase("diff", 2, 130, 33, 5, seed=1306, masked=False, adj_transpose=False, route=_LARGE, node="_PoolLargeFn"),
    AdjCase("diff", 2, 130, 3, 5, seed=1307, masked=False, hidden=7, route=_LARGE, node="_PoolLargeFn"),
    AdjCase("diff", 2, 80, 33, 5, seed=1308, masked=False, hidden=7, adj_transpose=False, normalize_loss=True,
            route=_LARGE, node="_PoolLargeFn"),
]
CASES = SMALL + LARGE


def _ids(cases):
    return [c.name for c in cases]


def _spy_routes(monkeypatch):
    """Record (pooler, route method) of every route method that answers, as test_gpu_dense_pooler_routes.py does."""
    from tgp.poolers import _DenseMLPPooling
    answered = []

    def spy(name):
        orig = getattr(_DenseMLPPooling, name)

        def wrapper(this, *a, **kw):
            r = orig(this, *a, **kw)
            if r is not None:
                answered.append((this, name))
            return r
        return wrapper
    for name in ROUTES:
        monkeypatch.setattr(_DenseMLPPooling, name, spy(name))
    return answered


def _pool_nodes(names):
    return [n for n in names if n.startswith(POOL_NODES)]


# ------------------------------------------------------------------------------------------------------------- the route
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_adjacency_that_requires_a_gradient_stays_on_the_fused_route(case, monkeypatch):
    import tgp.poolers as P
    from tgp import kernels as K
    B, N = case.adj.shape[:2]
    assert K.dense_pool_is_small(B, N, case.k, case.f) == (case in SMALL)
    assert not torch.equal(case.adj, case.adj.transpose(1, 2))
    answered = _spy_routes(monkeypatch)
    _, lv, names = case.run()
    assert lv["adj"].requires_grad and P._ADJ_GRAD
    assert [n for _, n in answered[:1]] == ([case.route] if case.route else []), answered
    assert len(_pool_nodes(names)) == 1 and _pool_nodes(names)[0].startswith(case.node), names
    # the flag off: the operator route, as before
    monkeypatch.setattr(P, "_ADJ_GRAD", False)
    del answered[:]
    _, _, names = case.run()
    assert not answered and not _pool_nodes(names), (answered, names)


# ------------------------------------------------------------------------------------------------------------- gradients
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_gradient_paths_with_the_adjacency_among_the_leaves(case):
    check_grad_paths(case.name, case.kernel, case.oracle, case.leaves)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [SMALL[1], SMALL[6], LARGE[1], LARGE[7]], ids=_ids([SMALL[1], SMALL[6], LARGE[1], LARGE[7]]))
def test_two_calls_on_fresh_copies_give_the_same_bits(case):
    def grads():
        outs, lv, _ = case.run()
        g = torch.Generator().manual_seed(5)
        total = sum((v * torch.randn(v.shape, generator=g).to(v.device)).sum() for v in outs.values())
        return torch.autograd.grad(total, [lv[n] for n in case.leaves])
    first, second = grads(), grads()
    for name, a, b in zip(case.leaves, first, second):
        assert torch.equal(a, b), name


# --------------------------------------------------------------------------------------------------------- the kernels alone
def _coefficient_inputs(B, N, K, seed, masked):
    """S (rows beyond a graph's size zero), a non-symmetric A and random upstream pieces, float64 on the host."""
    g = torch.Generator().manual_seed(seed)
    s = torch.softmax(torch.randn(B, N, K, generator=g, dtype=torch.float64) * 2, -1)
    if masked:
        sizes = torch.tensor(_ragged(B, N))
        s = s * (torch.arange(N).unsqueeze(0) < sizes.unsqueeze(1)).unsqueeze(-1)
    adj = (torch.rand(B, N, N, generator=g) * (torch.rand(B, N, N, generator=g) < 0.5)).double()
    pieces = dict(ga=torch.randn(B, K, K, generator=g).double(), g_raw=torch.randn(B, K, K, generator=g).double(),
                  g_terms=torch.randn(2, B, generator=g).double(), g_mean=torch.randn((), generator=g).double(),
                  g_link=torch.randn((), generator=g).double())
    return s, adj, pieces


def _check(got, want64, want32, what):
    e_k, e_32 = _rel(got.cpu().double(), want64), _rel(want32.double(), want64)
    bound = max(FACTOR * e_32, FLOOR)
    print(f"{what} | e_kernel {e_k:.2e} | e_restatement32 {e_32:.2e} | bound {bound:.2e}")
    assert bound <= CAP, (what, bound)
    assert e_k <= bound, (what, e_k, bound)
    worst = float((got.cpu().double() - want64).abs().max())
    assert worst <= 4 * bound * float(want64.abs().max()), (what, worst)


KERNEL_SHAPES = [(64, 12, 3), (64, 40, 12), (64, 64, 12), (64, 64, 3), (2, 80, 3), (2, 130, 33), (2, 130, 3), (2, 80, 33),
                 (2, 260, 32)]  # (the last: interior tiles, 16-byte operand loads and stores)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["mincut", "diff"])
@pytest.mark.parametrize("B,N,K", KERNEL_SHAPES, ids=[f"B{b}-N{n}-K{k}" for b, n, k in KERNEL_SHAPES])
def test_kernels_alone_against_the_float64_restatement(B, N, K, mode):
    from tgp import kernels as Kn
    dev = _dev()
    s, adj, pc = _coefficient_inputs(B, N, K, seed=B * 1000 + N + K, masked=N % 3 == 1)
    link_scale = 0.5
    g_r = pc["ga"] + pc["g_raw"]
    g_cut = (pc["g_terms"][0] + pc["g_mean"] / B) if mode == "mincut" else None
    g_link = pc["g_link"] if mode == "diff" else None
    f32 = lambda t: None if t is None else t.float()  # noqa: E731
    want64 = R.adj_grad(s, adj, g_r, g_cut, g_link, link_scale)
    want32 = R.adj_grad(f32(s), f32(adj), f32(g_r), f32(g_cut), f32(g_link), link_scale)
    m64, gamma64, _ = R.coefficients(s, adj, g_r, g_cut, g_link, link_scale)
    link_loss = (link_scale * torch.linalg.vector_norm(adj - s @ s.transpose(1, 2))).float().to(dev)
    sd, ad = s.float().to(dev), adj.float().to(dev)
    # the tiled kernel (any N, K): M and gamma given, q given or formed from S
    for q in (None, (sd * sd).sum(-1)):
        got = Kn.dense_pool_adj_grad(sd, ad, m64.float().to(dev), gamma=gamma64.float().to(dev) if mode == "mincut" else None,
                                     q=q, g_link=f32(g_link).to(dev) if mode == "diff" else None,
                                     link_loss=link_loss if mode == "diff" else None, link_scale=link_scale)
        _check(got, want64, want32, f"tiled {mode} B{B} N{N} K{K} q={'given' if q is not None else 'formed'}")
    # ... on S as a column block of a wider buffer and M as a block of taller one (the training step's operands)
    wide = torch.zeros(B, N, 2 * K + 3, device=dev)
    wide[:, :, K + 3:] = sd
    tall = torch.zeros(B, 2 * K + 1, K, device=dev)
    tall[:, K + 1:, :] = m64.float().to(dev)
    got = Kn.dense_pool_adj_grad(wide[:, :, K + 3:], ad, tall[:, K + 1:, :],
                                 gamma=gamma64.float().to(dev) if mode == "mincut" else None,
                                 g_link=f32(g_link).to(dev) if mode == "diff" else None,
                                 link_loss=link_loss if mode == "diff" else None, link_scale=link_scale)
    _check(got, want64, want32, f"tiled {mode} B{B} N{N} K{K} strided")
    if N <= 64 and K <= 32:  # one wave per graph: M and gamma are formed in the kernel
        raw = (s.transpose(1, 2) @ adj @ s).float().to(dev)
        got = Kn.dense_pool_adj_grad_small(
            sd, ad, f32(pc["ga"]).to(dev), f32(pc["g_raw"]).to(dev), raw,
            g_terms=f32(pc["g_terms"]).to(dev) if mode == "mincut" else None,
            g_mean_cut=f32(pc["g_mean"]).to(dev) if mode == "mincut" else None,
            g_link=f32(g_link).to(dev) if mode == "diff" else None, link_loss=link_loss if mode == "diff" else None,
            link_scale=link_scale)
        _check(got, want64, want32, f"one-wave {mode} B{B} N{N} K{K}")


def test_bad_arguments_are_refused_with_the_status_word():
    """Argument validation happens before any HIP call (runs without a GPU)."""
    import ctypes
    from tgp import _native
    lib = _native.lib()
    d = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(d)
    big = lib.tgp_dense_pool_adj_grad_f32
    assert big(p, 4, 0, None, p, 4, 0, None, None, None, None, 0.0, 2, -1, 4, p, p + 8, None) == -1
    assert b"tgp_dense_pool_adj_grad_f32" in lib.tgp_last_error()
    assert big(p, 4, 0, None, p, 4, 0, None, None, None, None, 0.0, 0, 8, 4, p, p + 8, None) == 0  # (an empty batch)
    assert big(None, 4, 0, None, p, 4, 0, None, None, None, None, 0.0, 2, 8, 4, p, p + 8, None) == -1  # no S
    assert big(p, 4, 0, None, p, 4, 0, None, None, None, None, 0.0, 2, 8, 0, p, p + 8, None) == -1  # K < 1
    assert big(p, 3, 0, None, p, 4, 0, None, None, None, None, 0.0, 2, 8, 4, p, p + 8, None) == -1  # row stride below K
    assert big(p, 4, 0, None, p, 4, 0, None, None, p, None, 0.0, 2, 8, 4, p, p + 8, None) == -1  # g_link without its loss
    assert b"link loss" in lib.tgp_last_error()
    assert big(p, 4, 0, None, p, 4, 0, None, None, None, None, 0.0, 2, 8, 4, p, p, None) == -1  # dA is the scratch
    assert big(p, 4, 0, None, p, 4, 0, None, None, None, None, 0.0, 2, 1 << 31, 4, p, p + 8, None) == -4  # TGP_ERR_RANGE
    small = lib.tgp_dense_pool_adj_grad_small_f32
    assert small(p, p, None, None, None, None, None, None, None, 0.0, 1e-8, 64, 65, 4, p + 8, None) == -1  # N > 64
    assert b"one wave per graph" in lib.tgp_last_error()
    assert small(p, p, None, None, None, None, None, None, None, 0.0, 1e-8, 64, 12, 33, p + 8, None) == -1  # K > 32
    assert small(p, p, None, None, None, None, p, None, None, 0.0, 1e-8, 64, 12, 4, p + 8, None) == -1  # cut term, no raw
    assert small(p, None, None, None, None, None, None, p, p, 0.0, 1e-8, 64, 12, 4, p + 8, None) == -1  # g_link, no A
    assert small(p, p, None, None, None, None, None, None, None, 0.0, 1e-8, 64, 12, 4, None, None) == -1  # no dA
    assert small(p, p, None, None, None, None, None, None, None, 0.0, 1e-8, 0, 12, 4, p + 8, None) == 0


@pytest.mark.gpu
def test_wrappers_refuse_operands_they_cannot_take():
    from tgp import kernels as Kn
    dev = _dev()
    s, adj, m = torch.rand(2, 70, 4, device=dev), torch.rand(2, 70, 70, device=dev), torch.rand(2, 4, 4, device=dev)
    with pytest.raises(ValueError, match="adj must be a contiguous float32"):
        Kn.dense_pool_adj_grad(s, adj.transpose(1, 2), m)
    with pytest.raises(ValueError, match="adj must be a contiguous float32"):
        Kn.dense_pool_adj_grad(s, adj.double(), m)
    with pytest.raises(ValueError, match="m must be"):
        Kn.dense_pool_adj_grad(s, adj, m[:, :3])
    with pytest.raises(ValueError, match="g_link needs"):
        Kn.dense_pool_adj_grad(s, adj, m, g_link=torch.ones((), device=dev))
    with pytest.raises(ValueError, match="N <= 64"):
        Kn.dense_pool_adj_grad_small(s, adj)
    with pytest.raises(ValueError, match="needs raw"):
        Kn.dense_pool_adj_grad_small(s[:, :60], adj[:, :60, :60].contiguous(), g_mean_cut=torch.ones((), device=dev))


# ---------------------------------------------------------------------------------------------------------------- memory
@pytest.mark.gpu
def test_backward_peak_memory_is_no_larger_than_on_the_operator_route(monkeypatch):
    import tgp.poolers as P
    case = AdjCase("mincut", 2, 260, 3, 5, seed=1401, masked=False, route=_LARGE, node="_PoolLargeFn")
    g = torch.Generator().manual_seed(5)
    ups = None

    def rise(flag):
        nonlocal ups
        monkeypatch.setattr(P, "_ADJ_GRAD", flag)
        peak = 0
        for _ in range(2):  # (the second, warm backward counts)
            outs, lv, names = case.run()
            assert bool(_pool_nodes(names)) == flag
            if ups is None:
                ups = [torch.randn(v.shape, generator=g).to(v.device) for v in outs.values()]
            total = sum((v * u).sum() for v, u in zip(outs.values(), ups))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            grads = torch.autograd.grad(total, [lv[n] for n in case.leaves])
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            del grads, total, outs, lv
        return peak
    on, off = rise(True), rise(False)
    print(f"backward peak rise: flag on {on} bytes, flag off {off} bytes")
    assert on <= off, (on, off)
    adj_bytes = case.adj.numel() * 4
    assert on < 2 * adj_bytes, (on, adj_bytes)  # dA is the only [B,N,N] tensor of the new path


# ----------------------------------------------------------------------------------------------------------- A is data
@pytest.mark.gpu
@pytest.mark.parametrize("case", [SMALL[0], SMALL[6], LARGE[1], LARGE[4]], ids=_ids([SMALL[0], SMALL[6], LARGE[1], LARGE[4]]))
def test_native_calls_are_unchanged_when_the_adjacency_is_data(case, monkeypatch):
    import tgp
    import tgp.poolers as P
    from tgp import _native as N

    def observe(flag):
        monkeypatch.setattr(P, "_ADJ_GRAD", flag)
        case.run(adj_grad=False)  # (what the package sets up once per process: unrecorded)
        recorder = _Recorder(N.lib(), N.SIGNATURES)
        with monkeypatch.context() as mp:
            mp.setattr(N, "_lib", recorder)
            tgp.clear_memos()
            outs, lv, names = case.run(adj_grad=False)
            forward, recorder.calls = recorder.calls, []
            sum(v.sum() for v in outs.values()).backward()
            torch.cuda.synchronize()
            assert lv["adj"].grad is None
            return forward, recorder.calls, _pool_nodes(names)
    on, off = observe(True), observe(False)
    assert on == off
    assert on[0] and on[1] and len(on[2]) == 1
    assert not any("adj_grad" in line for line in on[0] + on[1])


# ------------------------------------------------------------------------------------------------------------- the model
class _Stacked(torch.nn.Module):
    """MinCut, one dense propagation relu(A' X' W) in plain torch, DiffPool: the second level is handed the first level's
    pooled adjacency, an activation that requires a gradient."""

    def __init__(self, f, k1, h, k2):
        super().__init__()
        from tgp.poolers import get_pooler
        self.pool1 = get_pooler("mincut", in_channels=f, k=k1)
        self.lin = torch.nn.Linear(f, h, bias=False)
        self.pool2 = get_pooler("diff", in_channels=h, k=k2)

    def forward(self, x, adj):
        o1 = self.pool1(x=x, adj=adj)
        hid = torch.relu(o1.edge_index @ self.lin(o1.x))
        o2 = self.pool2(x=hid, adj=o1.edge_index)
        return o2.x, o2.edge_index, list(o1.loss.values()) + list(o2.loss.values())


def _stacked_oracle(x, adj, params, dtype):
    import tgp_oracle as O
    lv = {n: p.detach().cpu().to(dtype).requires_grad_(True) for n, p in params.items()}
    o1 = O.dense_pool("mincut", x.to(dtype), adj.to(dtype), None, None, [lv["pool1.selector.mlp.lins.0.weight"]],
                      [lv["pool1.selector.mlp.lins.0.bias"]])
    hid = torch.relu(o1["edge_index"] @ (o1["x"] @ lv["lin.weight"].t()))
    o2 = O.dense_pool("diff", hid, o1["edge_index"], None, None, [lv["pool2.selector.mlp.lins.0.weight"]],
                      [lv["pool2.selector.mlp.lins.0.bias"]])
    return o2["x"], o2["edge_index"], list(o1["loss"].values()) + list(o2["loss"].values()), lv


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,K1,K2,route", [(64, 40, 12, 3, _TRAIN), (2, 130, 80, 3, _LARGE)], ids=["one-wave", "large"])
def test_stacked_model_trains_on_the_fused_route(B, N, K1, K2, route, monkeypatch):
    import tgp.poolers as P
    F, H = 5, 6
    x, adj, _, _, _ = R.make_inputs(B, N, K1, F, seed=1500 + B)
    g = torch.Generator().manual_seed(9)
    wx, wa = torch.randn(B, K2, H, generator=g), torch.randn(B, K2, K2, generator=g)
    answered = _spy_routes(monkeypatch)

    def objective(xp, ap, losses, dt, dv):
        return (xp * wx.to(dv, dt)).sum() + (ap * wa.to(dv, dt)).sum() + sum(losses)

    def product(flag):
        monkeypatch.setattr(P, "_ADJ_GRAD", flag)
        torch.manual_seed(1500 + B)
        model = _Stacked(F, K1, H, K2).to(_dev()).train()
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        del answered[:]
        xp, ap, losses = model(x.to(_dev()), adj.to(_dev()))
        second = [n for this, n in answered if this is model.pool2]
        objective(xp, ap, losses, torch.float32, _dev()).backward()
        grads = {n: p.grad.detach().cpu().double().clone() for n, p in model.named_parameters()}
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        opt.step()
        for n, p in model.named_parameters():
            assert bool(torch.isfinite(p).all()) and not torch.equal(p, before[n]), n
        return grads, before, second

    g_on, params, second_on = product(True)
    g_off, params_off, second_off = product(False)
    assert second_on[:1] == [route] and not second_off, (second_on, second_off)
    assert all(torch.equal(params[n], params_off[n]) for n in params)  # (the same seeds: the same model)
    xp, ap, losses, lv = _stacked_oracle(x, adj, params, torch.float64)
    names = list(lv)
    want = dict(zip(names, torch.autograd.grad(objective(xp, ap, losses, torch.float64, "cpu"), [lv[n] for n in names])))
    assert set(want) == set(g_on)
    for n in names:
        assert bool(torch.isfinite(g_on[n]).all()), n
        e_on, e_off = _rel(g_on[n], want[n]), _rel(g_off[n], want[n])
        bound = max(FACTOR * e_off, FLOOR)
        print(f"stacked B{B} | {n} | e_on {e_on:.2e} | e_off {e_off:.2e} | bound {bound:.2e}")
        assert bound <= CAP, (n, bound)
        assert e_on <= bound, (n, e_on, bound)
        assert float((g_on[n] - want[n]).abs().max()) <= 4 * bound * float(want[n].abs().max()), n
