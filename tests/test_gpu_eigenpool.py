"""EigenPooling on the device: the modes, Reduce and Lift kernels of csrc/eigenpool.hip, the Connect identity, the
deterministic labeller and the routes, against the reference's stored results (tests/golden/golden_eigenpool_v1.pt, fed
in through ``labels=``) and against float64 restatements (tests/eigenpool_restatement.py)."""
import os

import pytest
import torch

import eigenpool_restatement as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BLOB = torch.load(os.path.join(HERE, "golden", "golden_eigenpool_v1.pt"), weights_only=True)
CASES, OPTS = BLOB["cases"], BLOB["opts"]
TOL = dict(rtol=1e-5, atol=1e-5)
# the gradient tolerance of tests/test_gpu_grad_paths.py
FACTOR, FLOOR, CAP = 16.0, 2e-6, 1e-3


def dev():
    return torch.device("cuda:0")


def on_device(c, opts, dtype=torch.float32, use_labels=True, batch="case"):
    from tgp.poolers import EigenPooling
    i, d = c["inputs"], dev()
    b = i["batch"] if batch == "case" else batch
    pooler = EigenPooling(**c["cfg"], **opts)
    x = i["x"].to(d, dtype).requires_grad_(True)
    kw = dict(labels=c["labels"].to(d)) if use_labels else {}
    out = pooler(x=x, adj=i["edge_index"].to(d), edge_weight=i["edge_weight"].to(d, dtype),
                 batch=None if b is None else b.to(d), **kw)
    return pooler, x, out


def check_adj(out, want, tol):
    if "dense" in want:
        assert out.edge_weight is None
        torch.testing.assert_close(out.edge_index.cpu().double(), want["dense"], **tol)
    else:
        assert torch.equal(out.edge_index.cpu(), want["edge_index"])
        torch.testing.assert_close(out.edge_weight.cpu().double(), want["edge_weight"], **tol)


# ------------------------------------------------------------------------------------------------ fixture parity
@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_the_reference_through_labels(name):
    from tgp.select import eigenpool_theta
    c = CASES[name]
    f64, f32 = c["f64"], c["expected"]
    pooler, x, out = on_device(c, OPTS[0])
    so = out.so
    assert "theta" not in so.__dict__ and so.theta_modes.dtype == torch.float32
    assert tuple(so.theta_modes.shape) == (x.size(0), c["cfg"]["num_modes"])
    assert so.theta_ptr.numel() == c["group_sizes"].numel() + 1 and so.theta_perm.numel() == x.size(0)
    assert torch.equal(so.s.cpu(), torch.nn.functional.one_hot(c["labels"], c["width"]).float())
    theta = eigenpool_theta(so)
    theta = theta if isinstance(theta, list) else [theta]
    assert len(theta) == len(f64["theta"])
    width, H = c["width"], c["cfg"]["num_modes"]
    slices = R.graph_slices(c["inputs"]["batch"], x.size(0))
    for gi, (t, t64, t32) in enumerate(zip(theta, f64["theta"], f32["theta"])):
        t = t.cpu().double()
        # the kernel computes in float64 and rounds once (6e-8 relative): compared with the float64 Theta
        torch.testing.assert_close(t, t64, **TOL)
        # against the reference's fp32 Theta only the triangle inequality holds: LAPACK's fp32 error grows with 1 / gap
        lab = c["labels"][slices[gi][0]:slices[gi][1]]
        for cl in range(width):
            nodes = (lab == cl).nonzero().view(-1)
            if nodes.numel():
                cols = [h * width + cl for h in range(H)]
                err = float((t[nodes][:, cols] - t32[nodes][:, cols].double()).abs().max())
                assert err <= float(c["err_ref"][gi * width + cl]) + 1e-5, (gi, cl, err)
    torch.testing.assert_close(out.x.detach().cpu().double().reshape(f64["x_pool"].shape), f64["x_pool"], **TOL)
    lift = pooler(x=out.x.detach(), so=so, batch=so.batch, lifting=True)
    torch.testing.assert_close(lift.cpu().double(), f64["lift"], **TOL)
    check_adj(out, f64["adj"][0], TOL)
    # d sum(x_pool^2) / dx against the stored float64 gradient, at fp32's own error on this data
    (g,) = torch.autograd.grad((out.x ** 2).sum(), x)
    g, g64 = g.cpu().double(), f64["grad_x"]
    th32 = torch.block_diag(*[t.float() for t in f64["theta"]])  # the float64 Theta rounded once, plain fp32 arithmetic
    x32 = c["inputs"]["x"].clone().requires_grad_(True)
    (g32,) = torch.autograd.grad(((th32.t() @ x32) ** 2).sum(), x32)
    e32 = float((g32.double() - g64).norm() / g64.norm())
    bound = max(FACTOR * e32, FLOOR)
    assert bound <= CAP
    e = float((g - g64).norm() / g64.norm())
    print(f"{name}: e_kernel {e:.3e} e_oracle32 {e32:.3e} bound {bound:.3e}")
    assert e <= bound and float((g - g64).abs().max()) <= 4 * bound * float(g64.abs().max())


@pytest.mark.parametrize("name", ["eig_batch6", "eig_planted", "eig_single20"])
def test_connector_options_of_the_fixture(name):
    c = CASES[name]
    for oi in (1, 2):
        b = c["inputs"]["batch"]
        if b is None and OPTS[oi]["sparse_output"]:
            b = torch.zeros(c["labels"].numel(), dtype=torch.long)  # (as the generator ran the reference)
        _, _, out = on_device(c, OPTS[oi], batch=b)
        check_adj(out, c["f64"]["adj"][oi], TOL)


# ------------------------------------------------------------------------------------------------ the modes kernel
def seeded_groups(sizes, seed, p=0.5, weighted=True):
    """One graph per entry of ``sizes`` (each its own cluster): symmetric, generic weights in [0.1, 1)."""
    g = torch.Generator().manual_seed(seed)
    eis, ews, bs, off = [], [], [], 0
    for gi, n in enumerate(sizes):
        up = torch.triu(torch.rand(n, n, generator=g) < p, 1)
        if n > 1:  # a path keeps every group connected
            up |= torch.diag(torch.ones(n - 1, dtype=torch.bool), 1)
        w = torch.triu(torch.rand(n, n, generator=g) * 0.9 + 0.1, 1) * up if weighted else up.float()
        a = w + w.t()
        idx = a.nonzero().t()
        eis.append(idx + off)
        ews.append(a[idx[0], idx[1]])
        bs.append(torch.full((n,), gi, dtype=torch.long))
        off += n
    return torch.cat(eis, 1), torch.cat(ews), torch.cat(bs)


def check_group_invariants(modes, a, normalized, H):
    """Residual, orthonormality and the sign rule of one group's modes [m, H] (float64 copies of the fp32 output)."""
    m = a.size(0)
    if m == 1:
        assert torch.equal(modes, a[0, 0].float().double().repeat(H).view(1, H))
        return None
    lap = R.laplacian(a, normalized)
    lam = torch.linalg.eigvalsh(lap)
    used = min(H, m)
    v = modes[:, :used]
    want = lam[:used]
    assert float((lap @ v - v * want.view(1, -1)).abs().max()) <= 1e-5  # ||L v - lambda v||_inf, lambda from eigvalsh
    torch.testing.assert_close(((lap @ v) * v).sum(0), want, **TOL)  # the Rayleigh quotients are the eigenvalues
    torch.testing.assert_close(v.t() @ v, torch.eye(used, dtype=torch.float64), **TOL)
    for h in range(used, H):  # beyond the group's size the last eigenvector repeats
        assert torch.equal(modes[:, h], modes[:, m - 1])
    assert bool((modes[0] >= 0).all())  # the lowest node's entry is never negative
    return lam


def run_selector(ei, ew, batch, labels, k, H, normalized=True, n=None):
    from tgp.select import EigenPoolSelect
    d = dev()
    sel = EigenPoolSelect(k=k, num_modes=H, normalized=normalized)
    return sel(edge_index=ei.to(d), edge_weight=None if ew is None else ew.to(d),
               batch=None if batch is None else batch.to(d), labels=None if labels is None else labels.to(d), num_nodes=n)


@pytest.mark.parametrize("normalized", [True, False])
def test_modes_kernel_against_float64_eigh_on_seeded_groups(normalized, monkeypatch):
    from tgp import kernels as K
    limit, H = K.eigenpool_max_group_nodes(), 5
    assert limit == 96
    sizes = [1, 2, 3, H - 1, H, H + 1, limit - 1, limit, limit + 1] * 3
    ei, ew, batch = seeded_groups(sizes, seed=11, p=0.35)
    calls = []
    real = torch.linalg.eigh
    monkeypatch.setattr(torch.linalg, "eigh", lambda a, *r, **kw: (calls.append(a.size(-1)), real(a, *r, **kw))[1])
    so = run_selector(ei, ew, batch, torch.zeros(batch.numel(), dtype=torch.long), 1, H, normalized)
    monkeypatch.undo()
    assert calls == [limit + 1] * 3  # only the over-limit groups took the composed route
    modes = so.theta_modes.cpu().double()
    outside = 0
    for gi, (lo, hi) in enumerate(R.graph_slices(batch, batch.numel())):
        a = R.dense_adjacency(ei, ew, lo, hi)
        lam = check_group_invariants(modes[lo:hi], a, normalized, H)
        if lam is None:
            continue
        m = hi - lo
        want, _ = R.cluster_modes(a, H, normalized)
        used = min(H + 1, m)
        if float((lam[1:used] - lam[:used - 1]).min()) < 1e-3 or float(want[0].abs().min()) < 1e-3:
            outside += 1  # the fixture's conditions: entries are compared only where they hold
            continue
        torch.testing.assert_close(modes[lo:hi], want, **TOL)
    print(f"normalized={normalized}: {outside} of {len(sizes)} groups outside the entry comparison")
    assert outside <= 0.05 * len(sizes)


def test_degenerate_groups_keep_the_invariants():
    """A disconnected cluster, a node of zero induced degree, an unweighted 4-cycle, an edgeless graph, an empty cluster
    in the middle of a graph and an empty graph in the middle of a batch: repeated eigenvalues leave the eigenvectors
    free, so only the residual, orthonormality and the sign rule are asked for."""
    H, k = 3, 3
    # graph 0 (7 nodes): cluster 0 = two disjoint edges (disconnected), cluster 1 EMPTY, cluster 2 = a triangle + a node
    # without induced edges (its only edge leaves the cluster); graph 1: no nodes; graph 2: an unweighted 4-cycle in
    # cluster 0 and two edgeless nodes in cluster 1; graph 3: three nodes, no edges at all, one cluster
    und = [(0, 1), (2, 3), (4, 5), (5, 6), (4, 6), (7, 0), (8, 9), (9, 10), (10, 11), (11, 8)]
    labels = torch.tensor([0, 0, 0, 0, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1, 0, 0, 0])
    batch = torch.tensor([0] * 8 + [2] * 6 + [3] * 3)
    ei = torch.tensor(und + [(b, a) for a, b in und]).t()
    ew = torch.ones(ei.size(1))
    for normalized in (True, False):
        so = run_selector(ei, ew, batch, labels, k, H, normalized)
        assert so.s.shape == (17, 3) and so.theta_ptr.numel() == 4 * k + 1
        sizes = (so.theta_ptr[1:] - so.theta_ptr[:-1]).cpu().tolist()
        assert sizes == [4, 0, 4, 0, 0, 0, 4, 2, 0, 3, 0, 0]
        modes = so.theta_modes.cpu().double()
        assert bool(torch.isfinite(modes).all())
        gid = batch * k + labels
        for g in gid.unique().tolist():
            nodes = (gid == g).nonzero().view(-1)
            lo, hi = int(nodes.min()), int(nodes.max()) + 1
            a = R.dense_adjacency(ei, ew, 0, 17)[nodes][:, nodes]
            check_group_invariants(modes[nodes], a, normalized, H)
        if normalized:  # a node without induced edges ends with a row of the identity: eigenvalue 1, not 0
            a = R.dense_adjacency(ei, ew, 0, 17)[4:8][:, 4:8]
            assert float(R.laplacian(a, True)[3, 3]) == 1.0 and float(R.laplacian(a, True)[3, :3].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ Reduce and Lift
def pool_inputs(F, H, n=301, G=23, seed=5):
    from tgp import kernels as K
    g = torch.Generator().manual_seed(seed)
    gid = torch.randint(0, G - 1, (n,), generator=g)  # interleaved in node order; the last group stays empty
    gid[gid == 3] = 4                                  # ... and so does one in the middle
    theta = torch.randn(n, H, generator=g)             # any values, not only orthonormal ones
    x = torch.randn(n, F, generator=g)
    y = torch.randn(G, H * F, generator=g)
    d = dev()
    groups = K.build_assign_index(gid.to(d), G)
    assert not torch.equal(groups.perm[:n].cpu().long(), torch.arange(n))
    return gid, theta, x, y, groups


@pytest.mark.parametrize("H", [1, 5, 7, 9])
@pytest.mark.parametrize("F", [1, 3, 32, 33, 130])
def test_reduce_and_lift_against_float64(F, H):
    from tgp import functions as Fn
    from tgp import kernels as K
    gid, theta, x, y, groups = pool_inputs(F, H)
    d, G = dev(), groups.num_targets
    gid_d, theta_d = gid.to(d, torch.int32), theta.to(d)
    pool = K.eigenpool_reduce(theta_d, groups, x.to(d))
    lift = K.eigenpool_lift(theta_d, gid_d, y.to(d), G)
    want_pool = torch.zeros(G, H, F, dtype=torch.float64).index_add_(
        0, gid, theta.double().unsqueeze(2) * x.double().unsqueeze(1)).view(G, H * F)
    want_lift = (theta.double().unsqueeze(2) * y.double().view(G, H, F)[gid]).sum(1)
    torch.testing.assert_close(pool.cpu().double(), want_pool, **TOL)
    torch.testing.assert_close(lift.cpu().double(), want_lift, **TOL)
    assert float(pool[3].abs().max()) == 0.0 and float(pool[G - 1].abs().max()) == 0.0  # empty groups: zero rows
    # the two kernels are each other's adjoint
    lhs = float((pool.cpu().double() * y.double()).sum())
    rhs = float((x.double() * lift.cpu().double()).sum())
    scale = float((want_pool.abs() * y.double().abs()).sum())
    assert abs(lhs - rhs) <= 1e-5 * scale
    # the same bits on every call
    assert torch.equal(pool, K.eigenpool_reduce(theta_d, groups, x.to(d)))
    # a batch with a long group has 4 or 16 waves share every group (max_len beyond 128 / 1024 rows): consecutive row
    # ranges folded in ascending order -- the same sums, the same bits on every call
    for max_len in (129, 1025):
        shared = K.eigenpool_reduce(theta_d, groups, x.to(d), max_len)
        torch.testing.assert_close(shared.cpu().double(), want_pool, **TOL)
        assert torch.equal(shared, K.eigenpool_reduce(theta_d, groups, x.to(d), max_len))
        assert float(shared[3].abs().max()) == 0.0
    assert torch.equal(lift, K.eigenpool_lift(theta_d, gid_d, y.to(d), G))
    # one autograd node each, the other kernel as its backward
    xg = x.to(d).requires_grad_(True)
    (gx,) = torch.autograd.grad((Fn.eigenpool_reduce(xg, theta_d, groups, gid_d) * y.to(d)).sum(), xg)
    assert torch.equal(gx, lift)
    yg = y.to(d).requires_grad_(True)
    (gy,) = torch.autograd.grad((Fn.eigenpool_lift(yg, theta_d, groups, gid_d) * x.to(d)).sum(), yg)
    assert torch.equal(gy, pool)


def test_reduce_forms_nothing_of_the_size_of_a_dense_theta():
    from tgp import kernels as K
    n, Kc, H, F = 4096, 64, 5, 32
    g = torch.Generator().manual_seed(2)
    d = dev()
    gid = torch.randint(0, Kc, (n,), generator=g).to(d)
    theta, x = torch.randn(n, H, generator=g).to(d), torch.randn(n, F, generator=g).to(d)
    groups = K.build_assign_index(gid, Kc)
    K.eigenpool_reduce(theta, groups, x)  # warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = K.eigenpool_reduce(theta, groups, x)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"warm Reduce: peak rise {rise} bytes (a dense Theta: {n * Kc * H * 4})")
    assert out.shape == (Kc, H * F) and rise < n * Kc * H * 4


# ------------------------------------------------------------------------------------------------ Connect
def test_connect_against_the_restatement_for_every_option():
    from tgp.connect import EigenPoolConnect
    from tgp.select import SelectOutput
    c = CASES["eig_planted"]  # self-loops, intra-cluster edges, empty clusters
    i, d = c["inputs"], dev()
    s = torch.nn.functional.one_hot(c["labels"], c["width"]).float().to(d)
    so = SelectOutput(s=s, batch=i["batch"].to(d))
    B = int(i["batch"].max()) + 1
    bp = torch.arange(B).repeat_interleave(c["width"]).to(d)
    for rsl in (True, False):
        for dn in (True, False):
            for ewn in (True, False):
                for sparse in (True, False):
                    opts = dict(remove_self_loops=rsl, degree_norm=dn, edge_weight_norm=ewn, sparse_output=sparse)
                    want = R.collapsed(i["x"], i["edge_index"], i["edge_weight"], i["batch"], c["labels"], c["width"], 1,
                                       True, opts)["adj"]
                    ref = R.reference_shape(i["x"], i["edge_index"], i["edge_weight"], i["batch"], c["labels"],
                                            c["width"], 1, True, opts)["adj"]
                    got_ei, got_w = EigenPoolConnect(**opts)(i["edge_index"].to(d), so, edge_weight=i["edge_weight"].to(d),
                                                             batch=i["batch"].to(d), batch_pooled=bp)
                    if sparse:
                        assert torch.equal(got_ei.cpu(), want[0]) and torch.equal(want[0], ref[0]), opts
                        torch.testing.assert_close(got_w.cpu().double(), want[1], **TOL)
                        torch.testing.assert_close(ref[1], want[1], rtol=1e-12, atol=1e-12)
                    else:
                        assert got_w is None
                        torch.testing.assert_close(got_ei.cpu().double(), want, **TOL)
                        torch.testing.assert_close(ref, want, rtol=1e-12, atol=1e-12)
                        assert float(got_ei.diagonal(dim1=-2, dim2=-1).abs().max()) == 0.0  # also without remove_self_loops


# ------------------------------------------------------------------------------------------------ the labeller
def same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def labels_of(so):
    return so.s.argmax(-1).cpu()


def test_labeller_partitions_are_valid_deterministic_and_numbered_by_lowest_node():
    c = CASES["eig_batch6"]
    i = c["inputs"]
    so = run_selector(i["edge_index"], i["edge_weight"], i["batch"], None, 4, 3)
    again = run_selector(i["edge_index"], i["edge_weight"], i["batch"], None, 4, 3)
    assert torch.equal(so.s, again.s) and torch.equal(so.theta_modes, again.theta_modes)  # the same bits
    assert so.s.shape == (i["batch"].numel(), 4)  # a batch always has width k
    assert torch.equal(so.s.sum(1).cpu(), torch.ones(i["batch"].numel()))
    lab = labels_of(so)
    for lo, hi in R.graph_slices(i["batch"], lab.numel()):
        l, n = lab[lo:hi], hi - lo
        if n <= 4:
            assert torch.equal(l, torch.arange(n))  # k >= n: one cluster per node
            continue
        assert sorted(l.unique().tolist()) == list(range(4))  # four non-empty clusters here
        firsts = [int((l == cl).nonzero()[0]) for cl in range(4)]
        assert firsts == sorted(firsts) and firsts[0] == 0  # numbered by their lowest member node


@pytest.mark.parametrize("name", [n for n, c in sorted(CASES.items()) if c["kind"] == "sklearn" and c["ref_matches_planted"]
                                  and c["cfg"]["k"] < c["labels"].numel()])
def test_labeller_recovers_the_planted_partition_where_the_reference_does(name):
    c = CASES[name]
    i, cfg = c["inputs"], c["cfg"]
    so = run_selector(i["edge_index"], i["edge_weight"], i["batch"], None, cfg["k"], cfg["num_modes"])
    lab = labels_of(so)
    assert so.s.size(1) == c["width"]
    for lo, hi in R.graph_slices(i["batch"], lab.numel()):
        assert same_partition(lab[lo:hi], c["planted"][lo:hi]), (name, lo)


def test_labeller_rules_that_do_not_depend_on_chance():
    ei, ew, batch = seeded_groups([6], seed=1)
    for k, fixed, width, want in ((1, False, 1, torch.zeros(6)), (6, False, 6, torch.arange(6)), (9, False, 6, torch.arange(6)),
                                  (9, True, 9, torch.arange(6)), (1, True, 1, torch.zeros(6))):
        from tgp.select import EigenPoolSelect
        so = EigenPoolSelect(k=k, num_modes=2)(edge_index=ei.to(dev()), edge_weight=ew.to(dev()), fixed_k=fixed)
        assert so.s.shape == (6, width), (k, fixed)
        assert torch.equal(labels_of(so), want.long())
    so = run_selector(ei, ew, None, None, 3, 2)
    assert so.s.shape == (6, 3) and sorted(labels_of(so).unique().tolist()) == [0, 1, 2]
    # no edges at all: the call returns a valid partition and finite modes
    from tgp.select import EigenPoolSelect
    so = EigenPoolSelect(k=2, num_modes=2)(edge_index=torch.zeros(2, 0, dtype=torch.long, device=dev()), num_nodes=5)
    assert so.s.shape == (5, 2) and torch.equal(so.s.sum(1).cpu(), torch.ones(5))
    assert bool(torch.isfinite(so.theta_modes).all()) and so.theta_modes.shape == (5, 2)
    # a batch: width k whatever the sizes; graphs of at most k nodes get one cluster per node
    ei, ew, batch = seeded_groups([2, 7, 1], seed=2)
    so = run_selector(ei, ew, batch, None, 3, 2)
    lab = labels_of(so)
    assert so.s.shape == (10, 3) and lab[:2].tolist() == [0, 1] and lab[9].item() == 0
    assert sorted(lab[2:9].unique().tolist()) == [0, 1, 2]


# ------------------------------------------------------------------------------------------------ routes
class Spy:
    def __init__(self, monkeypatch):
        from tgp import kernels as K
        self.calls = {"modes": 0, "reduce": 0, "lift": 0, "eigh": []}
        for name in ("modes", "reduce", "lift"):
            real = getattr(K, "eigenpool_" + name)
            monkeypatch.setattr(K, "eigenpool_" + name, self._wrap(name, real))
        real_eigh = torch.linalg.eigh
        monkeypatch.setattr(torch.linalg, "eigh",
                            lambda a, *r, **kw: (self.calls["eigh"].append(a.size(-1)), real_eigh(a, *r, **kw))[1])

    def _wrap(self, name, real):
        def f(*a, **kw):
            self.calls[name] += 1
            return real(*a, **kw)
        return f


def test_routes(monkeypatch):
    from tgp import kernels as K
    from tgp.poolers import EigenPooling
    from tgp.select import SelectOutput, eigenpool_theta
    spy = Spy(monkeypatch)
    c = CASES["eig_planted"]
    # groups inside the limit: the three kernels, no eigh
    pooler, x, out = on_device(c, OPTS[0])
    pooler(x=out.x.detach(), so=out.so, batch=out.so.batch, lifting=True)
    assert spy.calls == {"modes": 1, "reduce": 1, "lift": 1, "eigh": []}
    # a group over the limit: the kernel for the rest, eigh for that group alone
    limit = K.eigenpool_max_group_nodes()
    ei, ew, batch = seeded_groups([limit + 1, 5], seed=4, p=0.3)
    so = run_selector(ei, ew, batch, torch.zeros(limit + 6, dtype=torch.long), 1, 3)
    assert spy.calls["modes"] == 2 and spy.calls["eigh"] == [limit + 1]
    want = R.collapsed(torch.zeros(limit + 6, 1), ei, ew, batch, torch.zeros(limit + 6, dtype=torch.long), 1, 3)
    torch.testing.assert_close(so.theta_modes.cpu().double(), want["theta_modes"], **TOL)
    # an adjacency that is not symmetric: composed, reading the lower triangle as numpy's eigh does
    spy.calls["eigh"].clear()
    i = c["inputs"]
    ew_asym = i["edge_weight"].clone()
    gid_all = i["batch"] * 4 + c["labels"]
    keep = (i["edge_index"][0] != i["edge_index"][1]) & (gid_all[i["edge_index"][0]] == gid_all[i["edge_index"][1]])
    first = keep.nonzero()[0]  # an intra-cluster edge: its mate keeps the old weight
    ew_asym[first] += 0.25
    so = run_selector(i["edge_index"], ew_asym, i["batch"], c["labels"], 4, 5)
    sizes = c["group_sizes"]
    assert spy.calls["modes"] == 3 and sorted(spy.calls["eigh"]) == sorted(sizes[sizes > 1].tolist())
    want = R.collapsed(i["x"], i["edge_index"], ew_asym, i["batch"], c["labels"], 4, 5)
    torch.testing.assert_close(so.theta_modes.cpu().double(), want["theta_modes"], **TOL)
    # float64 inputs: composed throughout, float64 results
    before = dict(spy.calls, eigh=list(spy.calls["eigh"]))
    pooler, x, out = on_device(c, OPTS[0], dtype=torch.float64)
    lift = pooler(x=out.x.detach(), so=out.so, batch=out.so.batch, lifting=True)
    assert [spy.calls[k] for k in ("modes", "reduce", "lift")] == [before[k] for k in ("modes", "reduce", "lift")]
    assert out.x.dtype == torch.float64 and out.so.theta_modes.dtype == torch.float64 and lift.dtype == torch.float64
    torch.testing.assert_close(out.x.detach().cpu().reshape(c["f64"]["x_pool"].shape), c["f64"]["x_pool"], rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(lift.cpu(), c["f64"]["lift"], rtol=1e-9, atol=1e-9)
    check_adj(out, c["f64"]["adj"][0], dict(rtol=1e-9, atol=1e-9))
    # a SelectOutput built by user code with the reference's list (or dense) theta and no compact extras
    d = dev()
    _, _, out32 = on_device(c, OPTS[0])
    user = SelectOutput(s=out32.so.s.clone(), batch=out32.so.batch, theta=[t.clone() for t in eigenpool_theta(out32.so)])
    n_red, n_lift = spy.calls["reduce"], spy.calls["lift"]
    p = EigenPooling(**c["cfg"])
    xu, _ = p.reducer(i["x"].to(d), user, batch=i["batch"].to(d), return_batched=True)
    lu = p.lifter(xu, user, batch=i["batch"].to(d))
    assert (spy.calls["reduce"], spy.calls["lift"]) == (n_red, n_lift)
    torch.testing.assert_close(xu.cpu().double(), c["f64"]["x_pool"], **TOL)
    torch.testing.assert_close(lu.cpu().double(), c["f64"]["lift"], **TOL)
    c1 = CASES["eig_single20"]
    _, _, o1 = on_device(c1, OPTS[0])
    user1 = SelectOutput(s=o1.so.s.clone(), theta=eigenpool_theta(o1.so))
    x1, _ = EigenPooling(**c1["cfg"]).reducer(c1["inputs"]["x"].to(d), user1)
    torch.testing.assert_close(x1.cpu().double(), c1["f64"]["x_pool"], **TOL)
    torch.testing.assert_close(EigenPooling(**c1["cfg"]).lifter(x1, user1).cpu().double(), c1["f64"]["lift"], **TOL)


def test_cached_precoarsening_and_lifting_layouts(monkeypatch):
    from tgp.poolers import EigenPooling
    spy = Spy(monkeypatch)
    c = CASES["eig_batch3"]
    i, d = c["inputs"], dev()
    ei, ew, b, x = i["edge_index"].to(d), i["edge_weight"].to(d), i["batch"].to(d), i["x"].to(d)
    p = EigenPooling(**c["cfg"], cached=True)
    o1 = p(x=x, adj=ei, edge_weight=ew, batch=b)
    o2 = p(x=x * 2, adj=ei, edge_weight=ew, batch=b)
    assert spy.calls["modes"] == 2  # the labeller's embedding and the modes, once: the second call reuses the selection
    assert o2.so is o1.so and torch.equal(o2.x, o1.x * 2) and o2.edge_index is o1.edge_index
    B, Kc = 3, c["cfg"]["k"]
    assert o1.x.shape == (B, Kc, c["cfg"]["num_modes"] * x.size(1)) and o1.edge_index.shape == (B, Kc, Kc)
    flat = p(x=o1.x.reshape(B * Kc, -1), so=o1.so, batch=b, lifting=True)
    cube = p(x=o1.x, so=o1.so, batch=b, lifting=True)
    assert flat.shape == x.shape and torch.equal(flat, cube)
    # a copy of the SelectOutput (clone, pickle, .to) carries the extras, not the index objects: they are rebuilt from them
    twin = o1.so.clone()
    assert "_eig_cache" in o1.so.__dict__ and "_eig_cache" not in twin.__dict__
    assert torch.equal(p.reducer(x, twin, batch=b, return_batched=True)[0], o1.x)
    assert "_eig_cache" in twin.__dict__ and torch.equal(p.lifter(o1.x, twin, batch=b), cube)
    single = EigenPooling(k=3, num_modes=2)(x=x[:9], adj=ei[:, ei[0] < 9][:, ei[1][ei[0] < 9] < 9],
                                            edge_weight=ew[ei[0] < 9][ei[1][ei[0] < 9] < 9])
    assert torch.equal(EigenPooling(k=3, num_modes=2).reducer(x[:9], single.so.clone())[0], single.x)
    # pre-coarsening: width k also for one graph smaller than k, block-diagonal sparse connectivity
    c1 = CASES["eig_k_above_n"]
    i1 = c1["inputs"]
    pre = EigenPooling(**c1["cfg"]).precoarsening(edge_index=i1["edge_index"].to(d), edge_weight=i1["edge_weight"].to(d))
    assert pre.so.s.shape == (9, 12) and pre.edge_index.dim() == 2 and pre.edge_index.size(0) == 2
    assert pre.batch.numel() == 12 and int(pre.edge_index.max()) < 9
    free = EigenPooling(**c1["cfg"])(x=i1["x"].to(d), adj=i1["edge_index"].to(d), edge_weight=i1["edge_weight"].to(d))
    assert free.so.s.shape == (9, 9)  # without fixed_k one graph has width min(k, n)
    # every mode of a one-node cluster is the node's self-loop weight
    loops = i1["edge_index"][0] == i1["edge_index"][1]
    w = torch.zeros(9).index_add_(0, i1["edge_index"][0][loops], i1["edge_weight"][loops])
    assert torch.equal(free.so.theta_modes.cpu(), w.view(-1, 1).expand(9, 3))


def test_non_finite_edge_weights_stay_inside_their_graph():
    c = CASES["eig_batch3"]
    i, cfg = c["inputs"], c["cfg"]
    _, _, clean = on_device(c, OPTS[0])
    for bad in (float("nan"), float("inf")):
        ew = i["edge_weight"].clone()
        ei = i["edge_index"]
        in_g1 = ((i["batch"][ei[0]] == 1) & (ei[0] < ei[1])).nonzero().view(-1)
        e = int(in_g1[0])
        mate = int(((ei[0] == ei[1, e]) & (ei[1] == ei[0, e])).nonzero()[0])
        ew[e] = ew[mate] = bad
        c_bad = dict(c, inputs=dict(i, edge_weight=ew))
        _, _, out = on_device(c_bad, OPTS[0])
        torch.cuda.synchronize()
        assert torch.equal(out.x[0], clean.x[0]) and torch.equal(out.x[2], clean.x[2])
        assert torch.equal(out.edge_index[0], clean.edge_index[0]) and torch.equal(out.edge_index[2], clean.edge_index[2])
        assert not bool(torch.isfinite(out.x[1]).all() and torch.isfinite(out.edge_index[1]).all())
        # the labeller on the same input: it returns, and the graphs without the value keep their labels
        so = run_selector(ei, ew, i["batch"], None, cfg["k"], cfg["num_modes"])
        ok = run_selector(ei, i["edge_weight"], i["batch"], None, cfg["k"], cfg["num_modes"])
        torch.cuda.synchronize()
        keep = (i["batch"] != 1).to(dev())
        assert torch.equal(so.s[keep], ok.s[keep]) and torch.equal(so.theta_modes[keep], ok.theta_modes[keep])
        assert torch.equal(so.s.sum(1), torch.ones_like(so.s.sum(1)))
