"""BN-Pool's native sampled-edge loss (csrc/bnpool_edge.hip) against the composed expression in float64.

One batch of 70 nodes in 3 graphs: graph 0 a random directed list in shuffled order with duplicate edges, one self-loop,
node 3 that is only ever a destination and node 5 that appears only in the negative list; graph 1 random; graph 2 without
any edge or pair (its count clamps to 1, its term is 0).  Kmat is asymmetric and S peaked, so the logits spread to about
+-15 and both softplus branches run.  K walks the kernel's lane-group widths: 16-byte loads at K % 4 == 0 (1, 2, 4, ..,
64 lanes for K <= 4, 8, .., 256), scalar loads otherwise (1, 4, 16, 64 lanes for K <= 1, 4, 16, 256).

Tolerance per case: 4 x the error of the float32 composed expression on the same inputs against the float64 one (the
project's rule for a restated kernel) plus 8 float32 ulps of the result's largest magnitude."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = (30, 25, 15)
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 20, 31, 32, 33, 36, 63, 64, 65, 68, 127, 128, 129, 132, 255, 256)
ULPS = 8 * torch.finfo(torch.float32).eps


@pytest.fixture(autouse=True)
def _native_at_every_size(monkeypatch):
    """The size threshold below which the composed form is faster is a speed matter: here every size runs the kernels."""
    from tgp.utils import losses
    monkeypatch.setattr(losses, "BNPOOL_EDGE_MIN_EDGES", 0)


def make_batch(Kc, form="perm", seed=0):
    g = torch.Generator().manual_seed(seed)
    n0, n1, _ = SIZES
    rnd = lambda lo, hi, m: torch.randint(lo, hi, (m,), generator=g)
    src0, dst0 = rnd(0, n0, 90), rnd(0, n0, 90)
    keep = (src0 != 3) & (src0 != 5) & (dst0 != 5)  # node 3: no out-edge; node 5: in no positive edge
    pos = torch.cat([torch.stack([src0[keep], dst0[keep]]), torch.tensor([[7, 7, 7, 9], [3, 8, 8, 9]]),  # dup + self-loop
                     torch.stack([rnd(n0, n0 + n1, 60), rnd(n0, n0 + n1, 60)])], 1)
    neg = torch.cat([torch.stack([rnd(0, n0, 70), rnd(0, n0, 70)]), torch.tensor([[5, 11], [11, 5]]),
                     torch.stack([rnd(n0, n0 + n1, 40), rnd(n0, n0 + n1, 40)])], 1)
    pos = pos[:, torch.randperm(pos.size(1), generator=g)]
    if form == "sorted":
        pos = pos[:, pos[0].sort(stable=True)[1]]
    if form == "noneg":
        neg = neg[:, :0]
    batch = None if form == "nobatch" else torch.repeat_interleave(torch.arange(3), torch.tensor(SIZES))
    S = torch.softmax(torch.randn(sum(SIZES), Kc, generator=g) * 4.0, -1)
    Km = torch.randn(Kc, Kc, generator=g) * 6.0
    to = lambda t: None if t is None else t.to(DEV)
    return to(S), to(Km), to(pos), to(neg), to(batch)


def composed(S, Km, pos, neg, batch):
    e = torch.cat([pos, neg], 1)
    y = torch.cat([S.new_ones(pos.size(1)), S.new_zeros(neg.size(1))])
    bce = torch.nn.functional.binary_cross_entropy_with_logits(((S[e[0]] @ Km) * S[e[1]]).sum(-1), y, reduction="none")
    if batch is None:
        return bce.mean(), torch.tensor(float(e.size(1)), device=S.device, dtype=S.dtype)
    cnt = S.new_zeros(3).index_add_(0, batch[e[0]], torch.ones_like(bce)).clamp(min=1)
    return (S.new_zeros(3).index_add_(0, batch[e[0]], bce) / cnt).mean(), cnt


def values(fn, S, Km, *rest):
    """loss, count, dS with only S requiring a gradient, dK with only Kmat requiring one"""
    out = list(fn(S, Km, *rest))
    for which in (0, 1):
        leaves = [S.clone().requires_grad_(which == 0), Km.clone().requires_grad_(which == 1)]
        loss, _ = fn(*leaves, *rest)
        out.append(torch.autograd.grad(loss, leaves[which])[0])
    return out


@pytest.mark.parametrize("Kc,form", [(k, "perm") for k in WIDTHS] + [(20, f) for f in ("sorted", "nobatch", "noneg")])
def test_forward_and_gradients_against_float64(Kc, form):
    from tgp.utils.losses import bnpool_sparse_rec_loss
    S, Km, pos, neg, batch = make_batch(Kc, form)
    loss, _ = bnpool_sparse_rec_loss(S.clone().requires_grad_(), Km, pos, neg, batch)
    assert type(loss.grad_fn).__name__ == "_BNPoolEdgeRecFnBackward"
    got = values(bnpool_sparse_rec_loss, S, Km, pos, neg, batch)
    f32 = values(composed, S, Km, pos, neg, batch)
    ref = values(composed, S.double(), Km.double(), pos, neg, batch)
    assert got[1].dtype == torch.float32 and got[1].shape == ref[1].shape and torch.equal(got[1].double(), ref[1])
    for name, a, b, r in zip(("loss", "count", "dS", "dK"), got, f32, ref):
        err, base = float((a.double() - r).abs().max()), float((b.double() - r).abs().max())
        print(f"K={Kc} {form} {name}: native {err:.3e} composed-f32 {base:.3e} scale {float(r.abs().max()):.3e}")
        assert a.shape == r.shape and err <= 4 * base + ULPS * float(r.abs().max()), (name, err, base)


def test_same_bits_twice():
    from tgp.utils.losses import bnpool_sparse_rec_loss
    S, Km, pos, neg, batch = make_batch(20)
    a, b = (values(bnpool_sparse_rec_loss, S, Km, pos, neg.clone(), batch) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_no_edge_by_cluster_temporary():
    """Warm forward + backward at N = 4096, E' = 262144, K = 64: the peak rises by less than ONE E' x K float matrix."""
    from tgp.utils.losses import bnpool_sparse_rec_loss
    n, half, Kc = 4096, 131072, 64
    g = torch.Generator().manual_seed(1)
    S = torch.softmax(torch.randn(n, Kc, generator=g), -1).to(DEV).requires_grad_()
    Km = torch.randn(Kc, Kc, generator=g).to(DEV).requires_grad_()
    pos, neg = (torch.randint(0, n, (2, half), generator=g).to(DEV) for _ in range(2))
    peak = 0
    for step in range(2):  # the first call builds the indices and warms the allocator
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        bnpool_sparse_rec_loss(S, Km, pos, neg)[0].backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {peak / 2**20:.1f} MiB")
    assert peak < 2 * half * Kc * 4


def test_declines_take_the_composed_form(monkeypatch):
    from tgp.utils import losses
    from tgp.utils.losses import bnpool_sparse_rec_loss
    for Kc, dtype, shuffle in ((257, torch.float32, False), (20, torch.float64, False), (20, torch.float32, True),
                               (20, torch.float32, None)):
        S, Km, pos, neg, batch = make_batch(Kc)
        if shuffle is None:  # one sampled edge short of the size threshold
            monkeypatch.setattr(losses, "BNPOOL_EDGE_MIN_EDGES", pos.size(1) + neg.size(1) + 1)
        S, Km = S.to(dtype).requires_grad_(), Km.to(dtype)
        if shuffle:  # an unsorted batch vector
            batch = batch[torch.randperm(batch.numel(), device=DEV)]
        loss, count = bnpool_sparse_rec_loss(S, Km, pos, neg, batch, 3)
        want, want_count = composed(S, Km, pos, neg, batch)
        assert "BNPoolEdge" not in type(loss.grad_fn).__name__ and loss.dtype == dtype
        torch.testing.assert_close(loss, want, rtol=1e-6, atol=0)
        assert torch.equal(count, want_count)


def test_out_of_range_endpoint_is_skipped_and_reported():
    """An endpoint = N through the raw wrapper with hand-built indices: the row behind S's last (a sentinel of 1e30, real
    memory) is never read, the other edges give their loss, the status word is set; ``check=True`` raises."""
    from tgp import kernels as K
    n, Kc = 6, 8
    big = torch.full((n + 1, Kc), 1e30, device=DEV)
    big[:n] = torch.softmax(torch.randn(n, Kc, device=DEV), -1)
    S, Km = big[:n], torch.randn(Kc, Kc, device=DEV)
    T = torch.cat([S @ Km, big[n:]])[:n]
    pos = torch.tensor([[0, 0, 2, 4], [1, n, 3, 5]], device=DEV)  # sorted by source; the second edge ends at N
    neg = torch.tensor([[1], [2]], device=DEV)
    index = lambda ptr, E: K.AssignIndex(torch.tensor(ptr, dtype=torch.int32, device=DEV), None, E, n)
    pg, qg = index([0, 2, 2, 3, 3, 4, 4], 4), index([0, 0, 1, 1, 1, 1, 1], 1)
    node_loss, d_p, d_q, status = K.bnpool_edge_fwd(S, T, (pos, pg), (neg, qg))
    ok = torch.tensor([0, 2, 3], device=DEV)
    want, _ = composed(S.double(), Km.double(), pos[:, ok], neg, None)
    assert int(status) == 1 and float(d_p[1]) == 0.0
    torch.testing.assert_close(node_loss.double().sum() / 4, want, rtol=1e-5, atol=0)
    with pytest.raises(ValueError, match="out of range"):
        K.bnpool_edge_fwd(S, T, (pos, pg), (neg, qg), check=True)
    d_t, d_sv, status = K.bnpool_edge_bwd(S, T, (pos, pg, None), (neg, qg, None), d_p, d_q, torch.ones(1, device=DEV),
                                          want_dsv=False)
    assert int(status) == 2 and d_sv is None and bool(torch.isfinite(d_t).all()) and float(d_t[0].abs().max()) < 10


def test_pooler_unbatched():
    from tgp.poolers import BNPool
    _, _, pos, neg, batch = make_batch(6)
    x = torch.randn(sum(SIZES), 5, device=DEV)
    z = torch.rand(sum(SIZES), 5, device=DEV) * 0.9 + 0.05
    poolers, losses = [], []
    for dtype in (torch.float32, torch.float64):
        torch.manual_seed(3)
        p = BNPool(in_channels=5, k=6, batched=False).to(DEV).to(dtype)
        p.selector.sample_sticks = lambda q_z, z=z.to(dtype): z
        p.sample_negative_edges = lambda edge_index, b: neg
        poolers.append(p)
        losses.append(p(x=x.to(dtype), adj=pos, batch=batch).loss)
    for k in ("quality", "kl", "K_prior"):
        torch.testing.assert_close(losses[0][k].double(), losses[1][k], rtol=1e-5, atol=1e-5)
    sum(losses[0].values()).backward()
    for grad in (poolers[0].K.grad, poolers[0].selector.mlp.lins[0].weight.grad):
        assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().sum()) > 0
