"""GTVConv on the device: the whole layer against the fixture, the forward kernel against the float64 restatement at a
derived elementwise bound, the gradients one upstream path at a time, and the routes (dense on the sparse kernels, the
declines, determinism, memory)."""
import pytest
import torch

import gtv_restatement as R
from test_gpu_grad_paths import CAP, FACTOR, FLOOR, _graphs, check_grad_paths
from test_gtv_api import CASES, build_layer, fixture_error, layer_inputs

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _dev():
    return torch.device("cuda:0")


def _took(before, route):
    from tgp import kernels as K
    after = K.gtv_record()
    other = "composed" if route == "native" else "native"
    return after["route"] == route and after[route] > before[route] and after[other] == before[other]


# ------------------------------------------------------------------------------------------------ the layer, fixture
@pytest.mark.parametrize("name", sorted(CASES))
def test_layer_reproduces_the_fixture_on_the_native_route(name):
    from tgp import kernels as K
    c = CASES[name]
    before = K.gtv_record()
    with torch.no_grad():
        out = build_layer(c, _dev())(*layer_inputs(c, _dev()))
    assert _took(before, "native"), (before, K.gtv_record())
    e = fixture_error(out, c)
    bound = max(FACTOR * c["e_ref32"], FLOOR)
    print(f"{name}: e {e:.2e}, e_ref32 {c['e_ref32']:.2e}, bound {bound:.2e}")
    assert e <= bound, (name, e, bound)


# ------------------------------------------------------------------------ the forward kernel, elementwise and derived
def _batch(sizes, C, seed, weighted=True, directed=False, duplicates=False, isolated=False, scale=1.0):
    """(h [N,C] float32, edge_index, weights or None) of a batch of graphs; h is what the kernel and the oracle share."""
    _, ei, ew, _ = _graphs(sizes, 1, 4.0, seed, weighted, directed, duplicates, isolated)
    g = torch.Generator().manual_seed(seed + 17)
    return torch.randn(sum(sizes), C, generator=g) * scale, ei, ew


def _forward_bound(h, ei, w, bias, delta):
    """|out_ic - ref_ic| <= 2u (2 |h_ic| + |b_c| + delta (C + deg_i + 8) sum_out |w_e|): gamma_e |h_jc - h_ic| <= |w_e|
    whatever the clamp does, the distance is a C-term sum, the row a deg_i-term sum; relu and elu are 1-Lipschitz."""
    n, C = h.shape
    row, col = ei[0], ei[1]
    keep = (row != col) & (row >= 0) & (row < n) & (col >= 0) & (col < n)
    wk = (torch.ones(ei.size(1)) if w is None else w.abs())[keep].double()
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, row[keep], torch.ones_like(wk))
    wsum = torch.zeros(n, dtype=torch.float64).index_add_(0, row[keep], wk)
    b = torch.zeros(C, dtype=torch.float64) if bias is None else bias.abs().double()
    return 2 * U * (2 * h.abs().double() + b + (delta * (C + deg + 8) * wsum).unsqueeze(1))


def _check_forward(tag, h, ei, w, bias=None, mask=None, delta=1.0, eps=1e-3, act="relu", h_dev=None, ref_edges=None):
    from tgp import functions as Fn
    from tgp import kernels as K
    dev = _dev()
    hd = h.to(dev) if h_dev is None else h_dev
    out = Fn.gtv_propagate(hd, ei.to(dev), None if w is None else w.to(dev), None if bias is None else bias.to(dev),
                           None if mask is None else mask.to(dev), delta, eps, K.GTV_ACT_CODES[act])
    rei, rw = (ei, w) if ref_edges is None else ref_edges
    ref = R.propagate(h.double(), rei, None if rw is None else rw.double(), None if bias is None else bias.double(), mask,
                      delta, eps, R.ACTS[act])
    err = (out.cpu().double() - ref).abs()
    bound = _forward_bound(h, rei, rw, bias, delta)
    worst = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{tag}: max |err| {float(err.max()) if err.numel() else 0.0:.2e}, worst err/bound {worst:.3f}")
    assert bool((err <= bound).all()), (tag, worst)
    return out


SEVEN = [9, 1, 23, 2, 17, 5, 30]  # a 7-graph batch of unequal sizes
# both sides of every layout switch: the lane groups (32|33, 64|65, 128|129), the register count (256|257) and the chunked
# kernels (512|513), the vector loads (C % 4), and what the issue lists
WIDTHS = [1, 3, 4, 7, 8, 9, 32, 33, 64, 65, 128, 129, 130, 256, 257, 512, 513, 1100]


@pytest.mark.parametrize("C", WIDTHS)
def test_forward_kernel_widths(C):
    h, ei, w = _batch(SEVEN, C, 1000 + C, duplicates=C % 2 == 0)
    g = torch.Generator().manual_seed(C)
    bias = torch.randn(C, generator=g) * 0.3 if C % 3 else None
    _check_forward(f"C={C}", h, ei, w, bias, delta=0.311 if C % 2 else 1.0, act=("relu", "elu", "identity")[C % 3])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("C", [5, 8])
def test_forward_kernel_node_counts(n, C):
    h, ei, w = _batch([n], C, 2000 + n + C, weighted=C == 8, directed=True)
    if n == 1:
        ei, w = torch.zeros(2, 0, dtype=torch.long), None
    _check_forward(f"N={n} C={C}", h, ei, w, torch.linspace(-1, 1, C), act="elu")


def test_forward_kernel_edge_structures():
    C = 12
    h, ei, w = _batch(SEVEN, C, 3000)
    bias = torch.linspace(-0.5, 0.5, C)
    _check_forward("edgeless", h, torch.zeros(2, 0, dtype=torch.long), None, bias, act="elu")
    hi, eii, wi = _batch([20, 31], C, 3001, isolated=True)
    _check_forward("isolated nodes", hi, eii, wi, bias)
    path = torch.stack([torch.arange(40), torch.arange(1, 41)])  # 0 -> 1 -> ... -> 40: node 40 has no out-edge
    _check_forward("directed path", torch.randn(41, C, generator=torch.Generator().manual_seed(5)), path, None, None,
                   act="identity")
    loops = torch.arange(0, h.size(0), 3)
    ei2 = torch.cat([ei, torch.stack([loops, loops]), ei[:, ::4]], 1)
    w2 = torch.cat([w, torch.ones(loops.numel()), w[::4] * 0.5])
    _check_forward("duplicates and loops", h, ei2, w2, bias)
    order = torch.randperm(ei2.size(1), generator=torch.Generator().manual_seed(6))
    _check_forward("unsorted", h, ei2[:, order].contiguous(), w2[order].contiguous(), bias, delta=0.311)
    mask = torch.rand(h.size(0), generator=torch.Generator().manual_seed(7)) < 0.7
    out = _check_forward("mask", h, ei, w, bias, mask=mask, act="elu")
    assert float(out[~mask.to(out.device)].abs().max()) == 0.0


def test_forward_kernel_unaligned_rows_take_the_scalar_loads():
    """C % 4 == 0 with a base that is not 16-byte aligned: no vector load may touch it."""
    C = 16
    h, ei, w = _batch(SEVEN, C, 4000)
    flat = torch.zeros(h.numel() + 1, device=_dev())
    flat[1:] = h.to(_dev()).reshape(-1)
    view = flat[1:].view(h.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    _check_forward("unaligned", h, ei, w, None, h_dev=view)


def test_forward_kernel_skips_endpoints_out_of_range():
    from tgp import functions as Fn
    C = 8
    h, ei, w = _batch(SEVEN, C, 5000)
    n, dev = h.size(0), _dev()
    bad = torch.tensor([[0, n, 3, -1, 5, 2 ** 40], [n + 7, 1, -2, 4, 2 ** 33, 6]])
    at = torch.tensor([0, 9, 9, 30, 61, ei.size(1)])  # spliced in at several places, one at the end
    parts_e, parts_w, last = [], [], 0
    for k, pos in enumerate(at.tolist()):
        parts_e += [ei[:, last:pos], bad[:, k:k + 1]]
        parts_w += [w[last:pos], torch.tensor([0.7 + k])]
        last = pos
    ei2, w2 = torch.cat(parts_e + [ei[:, last:]], 1), torch.cat(parts_w + [w[last:]])
    assert ei2.size(1) == ei.size(1) + 6
    out = _check_forward("out of range", h, ei2, w2, None, ref_edges=(ei, w))
    clean = Fn.gtv_propagate(h.to(dev), ei.to(dev), w.to(dev), None, None, 1.0, 1e-3, 1)
    assert torch.equal(out, clean)
    # the kernel's own guard: destinations out of range under sources that are fine (the index is built from the sources)
    from tgp import kernels as K
    ei3 = ei.clone()
    cut = torch.tensor([1, 10, 40, ei.size(1) - 1])
    ei3[1, cut] = torch.tensor([-2, n, n + 7, 2 ** 33])
    kept = torch.ones(ei.size(1), dtype=torch.bool)
    kept[cut] = False
    e3, e4 = ei3.to(dev), ei[:, kept].contiguous().to(dev)
    got, d = K.gtv_edge_fwd(h.to(dev), e3[1].contiguous(), w.to(dev), K.sag_edge_group(e3, n, by_destination=False), None,
                            None, 1.0, 1e-3, 1, want_d=True)
    ref, _ = K.gtv_edge_fwd(h.to(dev), e4[1].contiguous(), w[kept].to(dev), K.sag_edge_group(e4, n, by_destination=False),
                            None, None, 1.0, 1e-3, 1)
    assert torch.equal(got, ref) and float(d.cpu()[cut].abs().max()) == 0.0
    # and through the backward: the removed edges get a zero weight gradient, the others the clean list's bits
    hd, wd = h.to(dev).requires_grad_(True), w2.to(dev).requires_grad_(True)
    hc, wc = h.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    up = torch.randn(h.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    g1 = torch.autograd.grad(Fn.gtv_propagate(hd, ei2.to(dev), wd, None, None, 1.0, 1e-3, 1), [hd, wd], up)
    g0 = torch.autograd.grad(Fn.gtv_propagate(hc, ei.to(dev), wc, None, None, 1.0, 1e-3, 1), [hc, wc], up)
    keep = torch.ones(ei2.size(1), dtype=torch.bool)
    keep[at + torch.arange(6)] = False
    assert torch.equal(g1[0], g0[0]) and torch.equal(g1[1].cpu()[keep], g0[1].cpu())
    assert float(g1[1].cpu()[~keep].abs().max()) == 0.0


def test_forward_kernel_with_eps_above_every_distance():
    C = 6
    h, ei, w = _batch(SEVEN, C, 6000, scale=0.01)
    _, d = R.distances(h.double(), ei)
    assert float(d.max()) < 0.5
    _check_forward("all clamped", h, ei, w, torch.linspace(-0.2, 0.2, C), eps=0.5, act="identity")


def test_wrappers_refuse_malformed_calls_on_device_tensors():
    from tgp import kernels as K
    dev = _dev()
    h, ei, w = _batch([10], 4, 1)
    h, ei, w = h.to(dev), ei.to(dev), w.to(dev)
    idx = K.sag_edge_group(ei, 10, by_destination=False)
    with pytest.raises(ValueError, match="gtv_edge_fwd"):
        K.gtv_edge_fwd(h, ei[1].contiguous(), w[:-1], idx, None, None, 1.0, 1e-3, 0)
    with pytest.raises(ValueError, match="gtv_edge_fwd"):
        K.gtv_edge_fwd(h.double(), ei[1].contiguous(), w, idx, None, None, 1.0, 1e-3, 0)
    with pytest.raises(ValueError, match="gtv_edge_fwd"):
        K.gtv_edge_fwd(h, ei[1].contiguous(), w, K.sag_edge_group(ei, 11, by_destination=False), None, None, 1.0, 1e-3, 0)


# ------------------------------------------------------------------------------------- gradients, one path at a time
class GradCase:
    """One layer call in training.  The data follows the fixture's separation rule: seeds are walked until no edge has a
    channel difference in (0, 1e-4) and no distance within 1e-4 eps of eps."""

    def __init__(self, name, sizes, *, seed, weighted=True, directed=False, duplicates=False, zero_edge=False, dense=False,
                 act="relu", bias=True, delta=1.0, eps=1e-3, f_in=5, f_out=6):
        self.name, self.act, self.delta, self.eps, self.dense = name, act, delta, eps, dense
        for s in range(seed, seed + 200):
            x, ei, ew, _ = _graphs(sizes, f_in, 4.0, s, weighted, directed, duplicates)
            g = torch.Generator().manual_seed(s + 1)
            weight = torch.randn(f_in, f_out, generator=g) * (2.0 / f_in) ** 0.5
            b = torch.randn(f_out, generator=g) * 0.3 if bias else None
            if duplicates:  # loops as well, and the list no longer sorted
                loops = torch.arange(0, x.size(0), 3)
                ei = torch.cat([ei, torch.stack([loops, loops])], 1)
                ew = torch.cat([ew, torch.rand(loops.numel(), generator=g) + 0.25])
                order = torch.randperm(ei.size(1), generator=g)
                ei, ew = ei[:, order].contiguous(), ew[order].contiguous()
            if zero_edge:  # two identical rows joined in both directions: d_e = 0
                x[1] = x[0]
                ei = torch.cat([torch.tensor([[0, 1], [1, 0]]), ei], 1)
                ew = torch.cat([torch.tensor([0.6, 0.9]), ew])
            self.mask = None
            if dense:
                B, n = len(sizes), max(sizes)
                adj = torch.zeros(B, n, n)
                off = 0
                for gi, m in enumerate(sizes):
                    sel = (ei[0] >= off) & (ei[0] < off + m)
                    adj[gi, ei[0, sel] - off, ei[1, sel] - off] = ew[sel]
                    off += m
                adj = adj + torch.diag_embed(torch.rand(B, n, generator=g) * 0.2 * (torch.rand(B, n, generator=g) < 0.5))
                self.mask = torch.arange(n).unsqueeze(0) < torch.tensor(sizes).unsqueeze(1)
                adj = adj * self.mask.unsqueeze(1) * self.mask.unsqueeze(2)
                xs = torch.zeros(B, n, f_in)
                off = 0
                for gi, m in enumerate(sizes):
                    xs[gi, :m] = x[off:off + m]
                    off += m
                x, ei, ew = xs, adj, None
                edges, _ = R.dense_edges(adj)
                hh = (x.double() @ weight.double()).reshape(B * n, -1)
            else:
                edges, hh = ei, x.double() @ weight.double()
            diff, d = R.distances(hh, edges)
            if not bool(((diff > 0) & (diff < 1e-4)).any()) and not bool(((d - eps).abs() < 1e-4 * eps).any()):
                break
        else:
            raise RuntimeError(f"{name}: no seed kept the kinks away")
        self.x, self.conn, self.ew, self.weight, self.bias = x, ei, ew, weight, b
        self.leaves = ["x", "weight"] + (["bias"] if bias else []) + (["edge_weight"] if ew is not None else [])

    def _act(self):
        return {"sigmoid": torch.sigmoid}.get(self.act) or R.ACTS[self.act]

    def oracle(self, dtype):
        lv = {"x": self.x.to(dtype).requires_grad_(True), "weight": self.weight.to(dtype).requires_grad_(True),
              "bias": None if self.bias is None else self.bias.to(dtype).requires_grad_(True),
              "edge_weight": None if self.ew is None else self.ew.to(dtype).requires_grad_(True)}
        conn = self.conn.to(dtype) if self.dense else self.conn
        out = R.layer(lv["x"], lv["weight"], lv["bias"], conn, lv["edge_weight"], self.mask, self.delta, self.eps,
                      self._act())
        return {"out": out}, lv

    def kernel(self):
        from tgp import kernels as K
        from tgp.mp import GTVConv
        dev = _dev()
        act = torch.sigmoid if self.act == "sigmoid" else self.act
        conv = GTVConv(self.x.size(-1), self.weight.size(1), bias=self.bias is not None, delta_coeff=self.delta,
                       eps=self.eps, act=act).to(dev)
        with torch.no_grad():
            conv.weight.copy_(self.weight)
            if self.bias is not None:
                conv.bias.copy_(self.bias)
        x = self.x.to(dev).requires_grad_(True)
        ew = None if self.ew is None else self.ew.to(dev).requires_grad_(True)
        before = K.gtv_record()
        out = conv(x, self.conn.to(dev), ew, None if self.mask is None else self.mask.to(dev))
        assert _took(before, "native"), self.name
        return {"out": out}, {"x": x, "weight": conv.weight, "bias": conv.bias, "edge_weight": ew}


GRAD_CASES = [
    GradCase("weighted-batch-relu", [14, 9, 20], seed=100, f_out=8),
    GradCase("wide-vector-rows-relu", [14, 9, 20], seed=120, f_out=260),
    GradCase("unweighted-directed-elu", [14, 9, 20], seed=150, weighted=False, directed=True, act="elu", delta=0.311),
    GradCase("duplicates-loops-identity", [14, 9, 20], seed=200, duplicates=True, act="identity"),
    GradCase("zero-distance-edge-elu", [14, 9, 20], seed=250, zero_edge=True, act="elu"),
    GradCase("dense-mask-relu", [9, 6, 8], seed=300, dense=True, directed=True),
    GradCase("not-fused-sigmoid", [14, 9, 20], seed=350, act="sigmoid", bias=False),
    GradCase("not-fused-tanh-wide", [14, 9, 20], seed=400, act="tanh", f_out=70),
    GradCase("clamped-eps-half", [14, 9, 20], seed=450, act="identity", eps=0.5, f_out=3),
]


@pytest.mark.parametrize("case", GRAD_CASES, ids=[c.name for c in GRAD_CASES])
def test_gradient_paths(case):
    check_grad_paths(case.name, case.kernel, case.oracle, case.leaves)


def test_wide_rows_backward_matches_the_composed_form():
    """The chunked backward kernels (C > 512) against torch's autograd of the composed form on the same device."""
    from tgp import functions as Fn
    from tgp.mp import gtv_propagate_composed
    dev = _dev()
    h, ei, w = _batch([12, 7], 600, 7000)
    bias = torch.linspace(-0.3, 0.3, 600)
    up = torch.randn(h.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    got, want = [], []
    for dtype, fn, into in ((torch.float32, None, got), (torch.float64, "composed", want)):
        lv = [t.to(dev, dtype).requires_grad_(True) for t in (h, w, bias)]
        if fn is None:
            out = Fn.gtv_propagate(lv[0], ei.to(dev), lv[1], lv[2], None, 0.311, 1e-3, 2)
        else:
            out = gtv_propagate_composed(lv[0], ei.to(dev), lv[1], lv[2], None, 0.311, 1e-3, torch.nn.functional.elu)
        into.extend(torch.autograd.grad(out, lv, up.to(dtype)))
    for name, g, ref in zip(("h", "edge_weight", "bias"), got, want):
        e = float(torch.linalg.vector_norm(g.double() - ref)) / float(torch.linalg.vector_norm(ref))
        print(f"wide {name}: e {e:.2e}")
        assert e <= 2e-4, (name, e)  # (the bound of the gradient cases: 16 x the float32 restatement's own 1.3e-5)


# ------------------------------------------------------------------------------------------------------- the routes
def test_dense_mode_equals_the_sparse_mode_on_its_nonzeros_bit_for_bit():
    from tgp import functions as Fn
    from tgp import kernels as K
    from tgp.mp import GTVConv
    dev = _dev()
    c = CASES["gtv_dense_batch_mask"]
    conv = build_layer(c, dev)
    x, adj, _, mask = layer_inputs(c, dev)
    B, n, _ = adj.shape
    ei, w = R.dense_edges(adj)
    with torch.no_grad():
        dense = conv(x, adj)
        sparse = conv(x.reshape(B * n, -1), ei, w)
        assert torch.equal(dense.reshape(B * n, -1), sparse)
        h = (x @ conv.weight).reshape(B * n, -1)
        masked = Fn.gtv_propagate(h, ei, w, conv.bias, mask.reshape(-1), conv.delta_coeff, conv.eps, K.GTV_ACT_CODES["relu"])
        assert torch.equal(conv(x, adj, mask=mask).reshape(B * n, -1), masked)
    assert isinstance(conv, GTVConv)


def test_dense_mode_with_a_float_mask_multiplies_after_the_kernel():
    dev = _dev()
    c = CASES["gtv_dense_batch_mask"]
    conv = build_layer(c, dev)
    x, adj, _, mask = layer_inputs(c, dev)
    with torch.no_grad():
        assert torch.equal(conv(x, adj, mask=mask.float()), conv(x, adj, mask=mask))


def test_dense_mode_with_adj_requiring_grad_takes_the_composed_form():
    """The reference differentiates every entry of ``adj``, the zero ones too: the matrix form, on the device.  Bound: the
    float32 reference's own error on this case (``e_ref32`` of the fixture: the same matrices, a_ii / eps cancelled
    between the degree and the entry) times FACTOR, as everywhere; normwise over all entries and entrywise at the zeros."""
    from tgp import kernels as K
    c = CASES["gtv_dense_batch_mask"]
    want = c["f64"]["grads"]["adj"]
    zero = c["inputs"]["adj"] == 0
    assert float(want[zero].abs().max()) > 0.0
    conv = build_layer(c, _dev())
    x, adj, _, mask = layer_inputs(c, _dev())
    adj.requires_grad_(True)
    before = K.gtv_record()
    out = conv(x, adj, mask=mask)
    assert _took(before, "composed")
    assert fixture_error(out, c) <= max(FACTOR * c["e_ref32"], FLOOR)
    (g,) = torch.autograd.grad(out, [adj], c["f64"]["upstream"].to(_dev(), torch.float32))
    g = g.cpu().double()
    e = float(torch.linalg.vector_norm(g - want)) / float(torch.linalg.vector_norm(want))
    bound = max(FACTOR * c["e_ref32"], FLOOR)
    print(f"dense adj gradient: e {e:.2e}, e_ref32 {c['e_ref32']:.2e}, bound {bound:.2e}")
    assert bound <= CAP and e <= bound
    assert float((g[zero] - want[zero]).abs().max()) <= 4 * bound * float(want.abs().max())


def test_two_calls_on_fresh_copies_give_equal_bits():
    from tgp import functions as Fn
    dev = _dev()
    h, ei, w = _batch(SEVEN + [40, 33], 24, 8000, duplicates=True)
    bias = torch.linspace(-0.3, 0.3, 24)
    up = torch.randn(h.shape, generator=torch.Generator().manual_seed(3))
    runs = []
    for _ in range(2):
        lv = [t.clone().to(dev).requires_grad_(True) for t in (h, w, bias)]
        out = Fn.gtv_propagate(lv[0], ei.clone().to(dev), lv[1], lv[2], None, 0.311, 1e-3, 2)
        runs.append([out.detach()] + list(torch.autograd.grad(out, lv, up.to(dev))))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_forward_allocates_nothing_of_size_edges_times_channels():
    from tgp.mp import GTVConv
    dev = _dev()
    n, E, C = 2000, 40000, 64
    g = torch.Generator().manual_seed(9)
    ei = torch.randint(0, n, (2, E), generator=g)
    ei = ei[:, torch.argsort(ei[0] * n + ei[1])].contiguous().to(dev)
    x, w = torch.randn(n, C, generator=g).to(dev), (torch.rand(E, generator=g) + 0.1).to(dev)
    conv = GTVConv(C, C).to(dev)
    with torch.no_grad():
        conv(x, ei, w)  # warms the edge index (and the matmul's workspace)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = conv(x, ei, w)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated(dev) - base
    limit = n * C * 4 + 2 * E * 4 + (1 << 20)
    print(f"forward peak extra {extra} bytes, limit {limit}, one E x C temporary {E * C * 4}")
    assert out.shape == (n, C) and extra <= limit, (extra, limit)


def test_declines_run_on_the_composed_form_and_match_the_restatement():
    from tgp import kernels as K
    c = CASES["gtv_undirected_weighted"]
    cfg = c["cfg"]
    dev = _dev()

    def want(dtype):
        return R.layer(c["inputs"]["x"].to(dtype), c["params"]["weight"].to(dtype), c["params"]["bias"].to(dtype),
                       c["inputs"]["edge_index"], c["inputs"]["edge_weight"].to(dtype), None, cfg.get("delta_coeff", 1.0),
                       cfg.get("eps", 1e-3), cfg["act"])

    # float64 on the device
    before = K.gtv_record()
    out = build_layer(c, dev, torch.float64)(*layer_inputs(c, dev, torch.float64))
    assert _took(before, "composed")
    torch.testing.assert_close(out.cpu(), want(torch.float64), rtol=1e-11, atol=1e-11)
    # host tensors
    before = K.gtv_record()
    out = build_layer(c)(*layer_inputs(c))
    assert _took(before, "composed")
    torch.testing.assert_close(out, want(torch.float32), rtol=1e-5, atol=1e-5)
    # a 2-D edge_weight [E, 1]
    x, ei, w, _ = layer_inputs(c, dev)
    before = K.gtv_record()
    out = build_layer(c, dev)(x, ei, w.unsqueeze(1))
    assert _took(before, "composed")
    torch.testing.assert_close(out.cpu(), want(torch.float32), rtol=1e-5, atol=1e-5)
    # float64 weights on float32 features
    before = K.gtv_record()
    build_layer(c, dev)(x, ei, w.double())
    assert _took(before, "composed")


def test_tvgnn_model_trains_one_step():
    """GTVConv -> GTVConv -> AsymCheegerCutPooling: a forward and a backward with finite gradients everywhere."""
    from tgp.mp import GTVConv
    from tgp.poolers import AsymCheegerCutPooling
    dev = _dev()
    torch.manual_seed(0)
    x, ei, ew, batch = _graphs([30, 21, 40], 8, 4.0, 77, True)
    x, ei, ew, batch = x.to(dev), ei.to(dev), ew.to(dev), batch.to(dev)
    c1, c2 = GTVConv(8, 16, act="elu").to(dev), GTVConv(16, 16, delta_coeff=0.311).to(dev)
    pool = AsymCheegerCutPooling(in_channels=16, k=5).to(dev).train()
    out = pool(x=c2(c1(x, ei, ew), ei, ew), adj=ei, edge_weight=ew, batch=batch)
    loss = out.x.pow(2).mean() + sum(out.loss.values())
    loss.backward()
    params = list(c1.parameters()) + list(c2.parameters()) + list(pool.parameters())
    assert params and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    assert float(c1.weight.grad.abs().max()) > 0.0
