"""BN-Pool on the GPU.

* Fixture parity: every pooler case of tests/golden/golden_bnpool_v1.pt (made by the reference,
  tests/golden/make_golden_bnpool.py) at the project's rtol = atol = 1e-5, the stored stick fractions injected through
  ``DPSelect.sample_sticks`` and, unbatched, the stored non-edges through ``BNPool.sample_negative_edges``: S, x, the
  pooled adjacency or edges (indices exact), batch and the three losses; the same under autograd.
* The native reconstruction loss (csrc/bnpool.hip: 32 x 32 logit tiles, four waves per block of 32 columns) against the
  float64 restatement (tests/bnpool_restatement.py, which multiplies S K S^T out) by maximum relative error at
  ROUTE_REL = 1e-5, the project's fp32 bound: a logit is a k-ordered fp32 fma chain of at most 33 x 33 terms, the loss a
  sum of at most 140^2 non-negative terms, so fp32's unit roundoff (6e-8) grows to about 1e-6.  The loss is judged
  relative to itself, gradients relative to their max-norm.  N in {1, 31, 32, 33, 64, 70, 130} straddles the tile edge
  (one row, below / exactly / above one tile, two tiles, ragged, five row blocks so that a wave takes two), K in
  {2, 5, 16, 33} is one stick, odd, half a k-tile, and two k-tiles with one column in the second; K = 130 takes the widest
  kernel.
* Gradients of each loss alone with tests/test_gpu_grad_paths.py's helper and constants, the restatement as the fp64 and
  fp32 oracle.
* Nothing N x N is formed: the peak of allocated memory around compute_loss and around its backward.
* Reproducibility bit for bit, and the negative-edge sampler's contract and host waits on device inputs."""
import os
import sys

import pytest
import torch
from torch.distributions import Beta

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bnpool_restatement as R  # noqa: E402
from test_bnpool_api import _seeded_batch, check_sampler_contract  # noqa: E402
from test_gpu_golden import check_output, check_so  # noqa: E402
from test_gpu_grad_paths import CAP, FACTOR, FLOOR, grad_path_errors  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = torch.load(os.path.join(HERE, "golden", "golden_bnpool_v1.pt"), weights_only=True)["cases"]
POOL = sorted(k for k, v in CASES.items() if v["kind"] == "pool")
LOSSES = ("quality", "kl", "K_prior")
ROUTE_REL = 1e-5
F64_REL = 1e-10


def _dev():
    return torch.device("cuda:0")


def _pooler(c, dev, dtype=torch.float32):
    from tgp.poolers import BNPool
    pooler = BNPool(**c["cfg"], batched=(c["alias"] == "bnpool")).to(dev).to(dtype)
    pooler.load_state_dict({k: v.to(dtype) for k, v in c["params"].items()})
    z = c["z"].to(dev).to(dtype)
    pooler.selector.sample_sticks = lambda q_z: z
    if c.get("neg_edge_index") is not None:
        neg = c["neg_edge_index"].to(dev)
        pooler.sample_negative_edges = lambda edge_index, batch: neg
    return pooler


def _call(pooler, inp, dev):
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    if "adj" in d:
        return pooler(x=d["x"], adj=d["adj"], mask=d.get("mask"))
    return pooler(x=d["x"], adj=d["edge_index"], edge_weight=d.get("edge_weight"), batch=d.get("batch"))


@pytest.mark.parametrize("name", POOL)
def test_fixture_parity(name):
    c = CASES[name]
    pooler = _pooler(c, _dev()).eval()
    with torch.no_grad():
        out = _call(pooler, c["inputs"], _dev())
    check_so(out.so, c["expected"]["so"], name)
    check_output(out, c["expected"], name)
    assert list(out.loss) == list(LOSSES)
    for k in LOSSES:
        assert out.loss[k].dim() == 0 and out.loss[k].dtype == torch.float32 and out.loss[k].is_cuda, k


@pytest.mark.parametrize("name", POOL)
def test_fixture_parity_under_autograd(name):
    c = CASES[name]
    pooler = _pooler(c, _dev())
    out = _call(pooler, c["inputs"], _dev())
    check_output(out, c["expected"], name + ".train")
    sum(out.loss.values()).backward()
    g = pooler.selector.mlp.lins[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0
    if c["cfg"].get("train_K", True):
        assert pooler.K.grad is not None and torch.isfinite(pooler.K.grad).all() and pooler.K.grad.abs().sum() > 0
    else:
        assert pooler.K.grad is None


def test_public_loss_functions_on_the_device():
    from test_bnpool_api import _function_values
    for tag in ("f32", "f64"):
        c = CASES[f"bnpool_functions_{tag}"]
        got = _function_values({k: v.to(_dev()) for k, v in c["inputs"].items()}, tag == "f32")
        for k, v in got.items():
            assert v.is_cuda and v.dtype == c["expected"][k].dtype, (tag, k)
            torch.testing.assert_close(v.cpu(), c["expected"][k], rtol=1e-5, atol=1e-5, msg=lambda m: f"{tag}.{k}: {m}")


# ------------------------------------------------------------------------------------------------------------ the route
def _route_inputs(N, Kc, seed, k_scale=1.0, peaked=False):
    """B = 3: graph 0 random, graph 1 complete (every entry nonzero), graph 2 edgeless; a directed adjacency with weights
    up to 3.2; an asymmetric K; a mask with holes and dirty padding (nonzero adjacency and S where the mask is off)."""
    g = torch.Generator().manual_seed(seed)
    B = 3
    adj = (torch.rand(B, N, N, generator=g) < 0.3).float() * (torch.rand(B, N, N, generator=g) * 3 + 0.2)
    adj[1] = torch.rand(N, N, generator=g) * 3 + 0.2
    mask = torch.ones(B, N, dtype=torch.bool)
    if N >= 4:
        mask[0, 1] = False
        mask[0, N - 2:] = False
        mask[2, torch.randperm(N, generator=g)[:N // 3]] = False
    pair = mask.unsqueeze(-1) & mask.unsqueeze(-2)
    adj[2] = adj[2] * (~pair[2])  # edgeless inside the mask, dirty outside
    S = torch.softmax(torch.randn(B, N, Kc, generator=g) * (4.0 if peaked else 1.0), -1)
    Km = torch.randn(Kc, Kc, generator=g) * k_scale
    return S, Km, adj, mask


def _max_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


class _Spy:
    """Counts the native entries of tgp.kernels and the composed form of tgp.utils.losses during a call."""

    def __init__(self, monkeypatch):
        from tgp import kernels as K
        from tgp.utils import losses as L
        self.count = {"bnpool_rec_fwd": 0, "bnpool_rec_bwd": 0, "_weighted_bce_terms": 0}
        for mod, n in ((K, "bnpool_rec_fwd"), (K, "bnpool_rec_bwd"), (L, "_weighted_bce_terms")):
            monkeypatch.setattr(mod, n, self._wrap(n, getattr(mod, n)))

    def _wrap(self, name, fn):
        def spy(*a, **kw):
            self.count[name] += 1
            return fn(*a, **kw)
        return spy


def _check_native(S, Km, adj, mask, spy):
    from tgp.utils.losses import bnpool_rec_loss_terms
    dev = _dev()
    s = S.to(dev).requires_grad_(True)
    k = Km.to(dev).requires_grad_(True)
    before = dict(spy.count)
    rec = bnpool_rec_loss_terms(s, k, adj.to(dev), None if mask is None else mask.to(dev))
    up = torch.linspace(0.5, 1.5, rec.numel(), device=dev)
    (rec * up).sum().backward()
    assert spy.count["bnpool_rec_fwd"] == before["bnpool_rec_fwd"] + 1
    assert spy.count["bnpool_rec_bwd"] == before["bnpool_rec_bwd"] + 1
    assert spy.count["_weighted_bce_terms"] == before["_weighted_bce_terms"]
    s64, k64 = S.double().requires_grad_(True), Km.double().requires_grad_(True)
    want = R.rec_terms(s64, k64, adj.double(), mask)
    (want * up.cpu().double()).sum().backward()
    assert rec.dtype == torch.float32 and rec.shape == want.shape
    errs = {"rec": float(((rec.detach().cpu().double() - want.detach()).abs() / want.detach().abs()).max()),
            "dS": _max_rel(s.grad, s64.grad), "dK": _max_rel(k.grad, k64.grad)}
    assert torch.isfinite(s.grad).all() and torch.isfinite(k.grad).all()
    if mask is not None:
        assert float(s.grad[~mask.to(dev)].abs().max() if (~mask).any() else 0.0) == 0.0  # no gradient into padded rows
    return errs


@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 70, 130])
def test_native_route_against_float64(N, monkeypatch):
    spy = _Spy(monkeypatch)
    for Kc in (2, 5, 16, 33):
        S, Km, adj, mask = _route_inputs(N, Kc, 1000 * N + Kc)
        errs = _check_native(S, Km, adj, mask, spy)
        print(f"N={N} K={Kc}", {k: f"{v:.2e}" for k, v in errs.items()})
        for k, v in errs.items():
            assert v <= ROUTE_REL, (N, Kc, k, v)
    S, Km, adj, _ = _route_inputs(N, 5, 77 + N)
    errs = _check_native(S, Km, adj, None, spy)  # no mask: every node counts
    for k, v in errs.items():
        assert v <= ROUTE_REL, (N, "nomask", k, v)


def test_native_route_widest_kernel(monkeypatch):
    spy = _Spy(monkeypatch)
    for N, Kc in ((33, 130), (70, 256), (40, 64), (40, 128)):
        errs = _check_native(*_route_inputs(N, Kc, N + Kc), spy)
        print(f"N={N} K={Kc}", {k: f"{v:.2e}" for k, v in errs.items()})
        for k, v in errs.items():
            assert v <= ROUTE_REL, (N, Kc, k, v)


def test_native_route_large_logits(monkeypatch):
    """K scaled so that |l| reaches about 30: softplus and sigmoid stay stable (expf / log1pf on -|l|)."""
    spy = _Spy(monkeypatch)
    S, Km, adj, mask = _route_inputs(70, 5, 5, k_scale=14.0, peaked=True)
    reach = float((S.double() @ Km.double() @ S.double().transpose(1, 2)).abs().max())
    assert 25.0 <= reach <= 60.0, reach
    errs = _check_native(S, Km, adj, mask, spy)
    print("large logits, max |l| =", reach, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= ROUTE_REL, (k, v)


def test_float64_device_inputs_take_the_composed_form(monkeypatch):
    from tgp.utils.losses import bnpool_rec_loss_terms
    spy = _Spy(monkeypatch)
    dev = _dev()
    S, Km, adj, mask = _route_inputs(70, 5, 9)
    rec = bnpool_rec_loss_terms(S.double().to(dev), Km.double().to(dev), adj.double().to(dev), mask.to(dev))
    assert spy.count == {"bnpool_rec_fwd": 0, "bnpool_rec_bwd": 0, "_weighted_bce_terms": 1}
    want = R.rec_terms(S.double(), Km.double(), adj.double(), mask)
    assert rec.dtype == torch.float64 and float(((rec.cpu() - want).abs() / want.abs()).max()) <= F64_REL
    # and a float64 pooler end to end
    c = CASES["bnpool_dense_inputs_mask_holes"]
    out = _call(_pooler(c, dev, torch.float64).eval(),
                {k: (v.double() if v.is_floating_point() else v) for k, v in c["inputs"].items()}, dev)
    from test_bnpool_restatement import restated_case
    _, ref = restated_case(c, torch.float64)
    assert spy.count["bnpool_rec_fwd"] == 0
    for k in LOSSES:
        assert out.loss[k].dtype == torch.float64
        assert abs(float(out.loss[k].detach()) - float(ref[k])) <= F64_REL * abs(float(ref[k])), k


def test_forward_and_backward_are_bit_reproducible():
    from tgp.utils.losses import bnpool_rec_loss_terms
    dev = _dev()
    S, Km, adj, mask = (t.to(dev) for t in _route_inputs(130, 16, 3))
    runs = []
    for _ in range(2):
        s, k = S.clone().requires_grad_(True), Km.clone().requires_grad_(True)
        rec = bnpool_rec_loss_terms(s, k, adj, mask)
        rec.sum().backward()
        runs.append((rec.detach(), s.grad, k.grad))
    for a, b in zip(*runs):  # (no float atomics in either direction)
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ gradients
def _mean_sticks(q_z):
    """A deterministic, differentiable stand-in for the draw: the posterior's mean alpha / (alpha + beta)."""
    return q_z.mean


def _grad_runs(N, Kc, f, seed):
    g = torch.Generator().manual_seed(seed)
    _, Km, adj, mask = _route_inputs(N, Kc, seed)
    x = torch.randn(3, N, f, generator=g)
    w = torch.randn(2 * (Kc - 1), f, generator=g) / f ** 0.5
    b = torch.randn(2 * (Kc - 1), generator=g) * 0.1
    cfg = dict(in_channels=f, k=Kc, K_mu=3.0, eta=0.5)
    names = ["x", "w", "b", "K"]

    def kernel():
        from tgp.poolers import BNPool
        dev = _dev()
        pooler = BNPool(**cfg).to(dev)
        with torch.no_grad():
            pooler.selector.mlp.lins[0].weight.copy_(w)
            pooler.selector.mlp.lins[0].bias.copy_(b)
            pooler.K.copy_(Km)
        pooler.selector.sample_sticks = _mean_sticks
        xd = x.to(dev).requires_grad_(True)
        out = pooler(x=xd, adj=adj.to(dev), mask=mask.to(dev))
        lin = pooler.selector.mlp.lins[0]
        return dict(out.loss), {"x": xd, "w": lin.weight, "b": lin.bias, "K": pooler.K}

    def oracle(dtype):
        xo, wo, bo, ko = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b, Km))
        alpha, beta = R.selector_params(xo, [wo], [bo])
        s = R.sticks_to_s(_mean_sticks(Beta(alpha, beta)), mask)
        eye = torch.eye(Kc, dtype=dtype)
        losses = R.bnpool_losses(s, ko, adj.to(dtype), mask, alpha, beta, torch.ones(Kc - 1, dtype=dtype),
                                 torch.ones(Kc - 1, dtype=dtype), 3.0 * eye - 3.0 * (1 - eye),
                                 torch.tensor(1.0, dtype=dtype), eta=0.5)
        return losses, {"x": xo, "w": wo, "b": bo, "K": ko}
    return kernel, oracle, names


@pytest.mark.parametrize("N,Kc", [(70, 16), (33, 5)], ids=["ragged_multi_block", "n33_k5"])
def test_gradient_paths(N, Kc, monkeypatch):
    spy = _Spy(monkeypatch)
    kernel, oracle, leaves = _grad_runs(N, Kc, 6, 40 + N)
    report = []
    name = f"bnpool_N{N}_K{Kc}"
    fails = grad_path_errors(name, kernel, oracle, leaves, report=report)
    for path, leaf, e_k, e_32 in report:
        print(f"{name} | {path} | {leaf} | e_kernel {e_k:.2e} | e_oracle32 {e_32:.2e} | bound "
              f"{max(FACTOR * e_32, FLOOR):.2e} (cap {CAP:g})")
    assert report and not fails, "\n".join(fails)
    assert {p for p, _, _, _ in report} == set(LOSSES)
    assert spy.count["bnpool_rec_bwd"] >= 1 and spy.count["_weighted_bce_terms"] == 0


# --------------------------------------------------------------------------------------------------------------- memory
def test_nothing_n_by_n_is_formed():
    """B = 4, N = 512, K = 16: around compute_loss and around its backward the peak of allocated memory stays below one
    quarter of one [B,N,N] float32 tensor (the route's own buffers are a few [B,N,K] of 3 % of it each, plus the tile
    records); the composed form on the same inputs exceeds it."""
    from tgp.poolers import BNPool
    from tgp.select import SelectOutput
    from tgp.utils.losses import weighted_bce_reconstruction_loss
    dev = _dev()
    g = torch.Generator().manual_seed(50)
    B, N, Kc = 4, 512, 16
    adj = ((torch.rand(B, N, N, generator=g) < 0.02).float() * (torch.rand(B, N, N, generator=g) + 0.5)).to(dev)
    mask = torch.ones(B, N, dtype=torch.bool, device=dev)
    mask[1, 400:] = False
    S = (torch.softmax(torch.randn(B, N, Kc, generator=g), -1).to(dev) * mask.unsqueeze(-1)).requires_grad_(True)
    q_z = Beta(torch.rand(B, N, Kc - 1, generator=g).to(dev) + 0.5, torch.rand(B, N, Kc - 1, generator=g).to(dev) + 0.5)
    pooler = BNPool(in_channels=4, k=Kc).to(dev)
    so = SelectOutput(s=S, in_mask=mask, q_z=q_z)
    limit = B * N * N * 4 // 4

    def peaks(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        value = fn()
        torch.cuda.synchronize()
        fwd = torch.cuda.max_memory_allocated() - base
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        value.backward()
        torch.cuda.synchronize()
        return fwd, torch.cuda.max_memory_allocated() - base

    fwd, bwd = peaks(lambda: sum(pooler.compute_loss(adj, mask, so).values()))
    print("native: peak rise forward", fwd, "backward", bwd, "limit", limit)
    assert fwd < limit and bwd < limit, (fwd, bwd, limit)
    assert torch.isfinite(S.grad).all() and S.grad.abs().sum() > 0 and pooler.K.grad.abs().sum() > 0
    n2 = mask.sum(-1) ** 2
    cf, cb = peaks(lambda: weighted_bce_reconstruction_loss(pooler.get_rec_adj(S), adj, mask, normalizing_const=n2))
    print("composed: peak rise forward", cf, "backward", cb)
    assert cf > limit and cb > limit, (cf, cb, limit)


# -------------------------------------------------------------------------------------------------------------- sampler
def _device_batch(count, seed):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(5, 41, (count,), generator=g).tolist()
    ei, batch = _seeded_batch(sizes, 0.25, seed + 1)
    return ei.to(_dev()), batch.to(_dev())


@pytest.mark.parametrize("method", ["auto", "sparse"])
@pytest.mark.parametrize("num,undirected", [(None, True), (None, False), (6, True)])
def test_sampler_contract_on_device_inputs(method, num, undirected):
    from tgp.utils.ops import batched_negative_edge_sampling
    ei, batch = _device_batch(64, 11)
    neg = batched_negative_edge_sampling(ei, batch, num_neg_samples=num, method=method, force_undirected=undirected)
    assert neg.is_cuda
    got, cap = check_sampler_contract(ei, batch, neg, num, undirected)
    assert int(got.sum()) >= int(cap.sum()) // 4  # (graphs of density 0.25 have room: most of the cap comes back)


@pytest.mark.parametrize("method", ["auto", "sparse"])
def test_sampler_host_waits_do_not_grow_with_the_batch(method, monkeypatch):
    """The proxy for host waits: every read-back of the sampler goes through ``ops._sampler_host_read`` (counted here),
    and outside it the call runs under ``torch.cuda.set_sync_debug_mode("warn")``, where every other operator that waits
    for the device (a boolean index, ``unique``, ``.item()``) raises a warning: the helper's calls plus those warnings
    are the call's host waits, and the number must be the same small constant for 8 graphs and for 64."""
    import warnings
    from tgp.utils import ops
    real = ops._sampler_host_read
    reads = []

    def counted(t):
        torch.cuda.set_sync_debug_mode("default")
        try:
            reads.append(1)
            return real(t)
        finally:
            torch.cuda.set_sync_debug_mode("warn")
    warm = _device_batch(4, 12)  # (the first call of a process may wait once more, for an operator's lazy set-up)
    ops.batched_negative_edge_sampling(warm[0], warm[1], force_undirected=True, method=method)
    monkeypatch.setattr(ops, "_sampler_host_read", counted)
    waits = []
    for count in (8, 64):
        ei, batch = _device_batch(count, 13)
        ops.batch_info(batch)  # (the batch facts are memoised per batch vector: not part of the sampler's own waits)
        torch.cuda.synchronize()
        del reads[:]
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                neg = ops.batched_negative_edge_sampling(ei, batch, force_undirected=True, method=method)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        sync_warnings = [w for w in seen if "called a synchronizing" in str(w.message)]
        waits.append((len(reads), len(sync_warnings)))
        for w in sync_warnings:
            print(count, "graphs:", w.filename.rsplit("/", 1)[-1], w.lineno, str(w.message)[:60])
        assert neg.size(1) > 0
    print(method, "host reads / sync warnings for 8 and 64 graphs:", waits)
    assert waits[0] == waits[1]
    assert waits[0][0] == 1 and 1 <= waits[0][1] <= 2  # (the boolean index that sizes the result; ``unique`` when drawing)


def test_unbatched_pooler_draws_its_own_negative_edges(monkeypatch):
    """The unbatched mode end to end with the project's sampler (no injected non-edges): the sampler is asked once, for
    undirected pairs, its pairs satisfy the contract, and the three losses are finite with gradients to K."""
    from tgp.utils import ops
    import tgp.poolers as P
    c = CASES["bnpool_u_default"]
    dev = _dev()
    pooler = _pooler(dict(c, neg_edge_index=None), dev)
    seen = []
    real = ops.batched_negative_edge_sampling

    def spy(edge_index, batch, **kw):
        out = real(edge_index, batch, **kw)
        seen.append((kw, out))
        return out
    monkeypatch.setattr(P, "batched_negative_edge_sampling", spy)
    out = _call(pooler, c["inputs"], dev)
    assert len(seen) == 1 and seen[0][0] == dict(num_neg_samples=None, force_undirected=True)
    got, _ = check_sampler_contract(c["inputs"]["edge_index"], c["inputs"]["batch"], seen[0][1], None, True)
    assert int(got.sum()) > 0
    for k in LOSSES:
        assert out.loss[k].dim() == 0 and out.loss[k].dtype == torch.float32 and torch.isfinite(out.loss[k]), k
    sum(out.loss.values()).backward()
    assert torch.isfinite(pooler.K.grad).all() and pooler.K.grad.abs().sum() > 0
