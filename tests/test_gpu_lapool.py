"""LaPool on the GPU: the reference's fixtures, the selector's three operators one by one against float64, dense and
sparse inputs at the sizes where the kernels change path, ties and degenerate inputs, the backward, and memory.

Bounds.  Fixture parity is ``rtol = atol = 1e-5``.  Every other float comparison uses the bound of
test_gpu_grad_paths.py: with e = ||y - y_64|| / ||y_64||, e_kernel <= max(FACTOR e_composed32, FLOOR) and
max|y - y_64| <= 4 bound max|y_64|, the bound itself at most CAP; the composed form is tests/lapool_restatement.py in
float32 on the host.  Leader flags are compared bit for bit with ``leaders_from`` on the kernel's own v.

The native kernels have no size cut (a wave per row, a workgroup per graph for the columns); the sizes below cross a
wave (64 leaders or rows), a 256-column chunk of A and a 256-row scan step.  The one route choice is on the host: an
edge list with ascending sources runs on its CSR offsets, any other on the by-source index; both are run and compared."""
import functools
import os

import pytest
import torch

import lapool_restatement as R
from test_gpu_grad_paths import CAP, FACTOR, FLOOR, check_grad_paths

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_lapool_v1.pt"), weights_only=True)["cases"]
DEV = torch.device("cuda:0")


def _rel(a, b):
    return float(torch.linalg.vector_norm(a - b)) / max(float(torch.linalg.vector_norm(b)), 1e-300)


def _within(what, got, want64, composed32):
    got, want64, composed32 = got.detach().cpu().double(), want64.detach().cpu().double(), composed32.detach().cpu().double()
    assert got.shape == want64.shape, f"{what}: shape {tuple(got.shape)} against {tuple(want64.shape)}"
    e_k, e_32 = _rel(got, want64), _rel(composed32, want64)
    bound = max(FACTOR * e_32, FLOOR)
    print(f"{what}: e_kernel {e_k:.3e}, e_composed32 {e_32:.3e}, bound {bound:.3e}")
    assert bound <= CAP, f"{what}: the bound {bound:.3e} exceeds {CAP:g} (ill-conditioned data)"
    assert e_k <= bound, f"{what}: e_kernel {e_k:.3e} above the bound {bound:.3e} (e_composed32 {e_32:.3e})"
    worst = float((got - want64).abs().max())
    assert worst <= 4 * bound * float(want64.abs().max()), f"{what}: max |y - y_64| = {worst:.3e}"


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def dense_input(name):
    """(x [B,N,F], adj [B,N,N], mask or None) on the host."""
    B, N, F, p, seed, kind = {"n37f5": (3, 37, 5, 0.15, 11, "random_mask"), "n64f64": (3, 64, 64, 0.1, 12, None),
                              "n300f70": (2, 300, 70, 0.02, 13, "sizes"), "special": (3, 16, 6, 0.3, 14, "special"),
                              "directed": (2, 21, 8, 0.2, 15, "directed")}[name]
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(B, N, N, generator=g) < p).float() * (torch.rand(B, N, N, generator=g) + 0.1)
    if kind != "directed":
        a = torch.triu(a, 1)
        a = a + a.transpose(1, 2)
    x = torch.randn(B, N, F, generator=g)
    mask = None
    if kind == "random_mask":
        mask = torch.rand(B, N, generator=g) < 0.8
    elif kind == "sizes":
        mask = torch.arange(N).unsqueeze(0) < torch.tensor([300, 257]).unsqueeze(1)
    elif kind == "special":  # a full graph, a 1-node graph, an empty graph
        mask = torch.zeros(B, N, dtype=torch.bool)
        mask[0] = True
        mask[1, 5] = True
    return x, a, mask


@functools.lru_cache(maxsize=None)
def sparse_input(name):
    """(x [n,F], edge_index, edge_weight, batch) on the host: a sorted batch with directed edges, duplicates, self-loops,
    an isolated node, and a last graph without edges (all its nodes lead: k_b = 70 there)."""
    sizes, F, seed = {"sizes": ([1, 2, 63, 64, 65, 70], 7, 21), "wide": ([3, 130, 40], 68, 22)}[name]
    g = torch.Generator().manual_seed(seed)
    xs, eis, bs, off = [], [], [], 0
    for gi, n in enumerate(sizes):
        xs.append(torch.randn(n, F, generator=g))
        bs.append(torch.full((n,), gi, dtype=torch.long))
        if gi < len(sizes) - 1 and n > 1:
            a = torch.rand(n, n, generator=g) < min(0.5, 4.0 / n)
            a[:, n - 1] = False
            a[n - 1, :] = False  # the graph's last node is isolated
            ei = a.nonzero().t()  # directed, self-loops included
            dup = ei[:, torch.randperm(ei.size(1), generator=g)[: max(1, ei.size(1) // 5)]]
            eis.append(torch.cat([ei, dup], 1) + off)
        off += n
    ei = torch.cat(eis, 1)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    ew = torch.rand(ei.size(1), generator=g) + 0.1
    ew[3] = 0.0
    return torch.cat(xs), ei.contiguous(), ew, torch.cat(bs)


def _ptr(batch):
    sizes = torch.bincount(batch)
    return torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


# ------------------------------------------------------------------------------------------------ 1. fixture parity
def _run_case(case, requires_grad=False):
    from tgp.poolers import LaPooling
    kw = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in case["inputs"].items()}
    x = kw.pop("x").clone().requires_grad_(requires_grad)
    if "edge_index" in kw:
        kw["adj"] = kw.pop("edge_index")
    return x, LaPooling(**case["cfg"]).to(DEV).eval()(x=x, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_parity(name):
    case = CASES[name]
    exp = case["expected"]
    with torch.no_grad():
        _, out = _run_case(case)
    so = out.so
    assert torch.equal(so.leader_mask.cpu(), exp["so"]["leader_mask"])
    assert so.s.shape == exp["so"]["s"].shape
    tol = dict(rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(so.s.cpu(), exp["so"]["s"], **tol)
    torch.testing.assert_close(out.x.cpu(), exp["x"], **tol)
    if exp["edge_index"].is_floating_point():  # a pooled dense adjacency
        torch.testing.assert_close(out.edge_index.cpu(), exp["edge_index"], **tol)
        assert out.edge_weight is None and exp["edge_weight"] is None
    else:
        assert torch.equal(out.edge_index.cpu(), exp["edge_index"])
        torch.testing.assert_close(out.edge_weight.cpu(), exp["edge_weight"], **tol)
    if exp["batch"] is None:
        assert out.batch is None
    else:
        assert torch.equal(out.batch.cpu(), exp["batch"])
    if "in_mask" in exp["so"]:
        assert torch.equal(so.in_mask.cpu(), exp["so"]["in_mask"])


# ------------------------------------------------------------------------------------- 2.-4. operators one by one
@pytest.mark.parametrize("name", ["n37f5", "n64f64", "n300f70", "special", "directed"])
def test_dense_operators(name):
    from tgp import kernels as K
    x, a, mask = dense_input(name)
    xd, ad, md = _dev(x, a, mask)
    # (a) v
    v = K.lapool_variation(xd, ad, md)
    _within(f"{name} v", v, R.variation(x.double(), a.double(), mask), R.variation(x, a, mask))
    if mask is not None:
        assert torch.equal(v[~md], torch.zeros_like(v[~md]))
    # (b) flags: the same comparison of the same floats
    lead = K.lapool_leaders(v, ad, md)
    want = R.leaders_from(v, ad, md)
    assert torch.equal(lead.flags, want)
    k = want.sum(1)
    assert torch.equal(lead.k.long(), k) and lead.k_max == int(k.max())
    # (c) S for that leader mask
    s, _ = K.lapool_assign(xd, lead)
    flags = want.cpu()
    s64, s32 = R.assign(x.double(), flags, mask=mask), R.assign(x, flags, mask=mask)
    _within(f"{name} S", s, s64, s32)
    assert torch.equal(s.cpu() == 0, s64 == 0) and torch.equal(s.cpu() == 1, s64 == 1)
    # a caller's own leader mask takes the same kernels (no fall-back: the mask is taken as it is)
    again = K.lapool_columns(want, mask=md)
    assert torch.equal(again.col_of, lead.col_of) and torch.equal(K.lapool_assign(xd, again)[0], s)


def test_dense_vector_and_element_loads_agree():
    """The 16-byte path (N % 4 == 0, aligned) and the element path add in the same order: the same bits on the same
    numbers.  A batch whose storage starts 4 bytes into an allocation takes the element path."""
    from tgp import kernels as K
    x, a, _ = dense_input("n64f64")
    xd, ad = _dev(x, a)
    shifted = torch.empty(a.numel() + 1, device=DEV)[1:].view_as(a).copy_(ad)
    xs = torch.empty(x.numel() + 1, device=DEV)[1:].view_as(x).copy_(xd)
    assert shifted.data_ptr() % 16 == 4 and xs.data_ptr() % 16 == 4 and ad.data_ptr() % 16 == 0
    v0, v1 = K.lapool_variation(xd, ad), K.lapool_variation(xs, shifted)
    assert torch.equal(v0, v1)
    lead = K.lapool_leaders(v0, ad)
    assert torch.equal(K.lapool_assign(xd, lead)[0], K.lapool_assign(xs, lead)[0])


@pytest.mark.parametrize("name", ["sizes", "wide"])
def test_sparse_operators(name):
    from tgp import kernels as K
    x, ei, ew, batch = sparse_input(name)
    xd, eid, ewd, bd = _dev(x, ei, ew, batch)
    ptr = _ptr(batch).to(DEV)
    v = K.lapool_variation(xd, edge_index=eid, edge_weight=ewd)
    _within(f"{name} v", v, R.variation(x.double(), edge_index=ei, edge_weight=ew.double()),
            R.variation(x, edge_index=ei, edge_weight=ew))
    lead = K.lapool_leaders(v, edge_index=eid, batch=bd, ptr=ptr)
    want = R.leaders_from(v, edge_index=eid, batch=bd)
    assert torch.equal(lead.flags, want)
    k = torch.zeros(ptr.numel() - 1, dtype=torch.long, device=DEV).index_add_(0, bd, want.long())
    assert torch.equal(lead.k.long(), k) and lead.k_max == int(k.max())
    if name == "sizes":
        assert k.tolist()[-1] == 70 and k.tolist()[0] == 1  # the edgeless graph: every node leads, beyond one wave
        assert bool(want[ptr[1:-1] + torch.bincount(batch)[1:].to(DEV) - 1].all())  # isolated nodes lead
    s, _ = K.lapool_assign(xd, lead)
    flags = want.cpu()
    s64, s32 = R.assign(x.double(), flags, batch=batch), R.assign(x, flags, batch=batch)
    _within(f"{name} S", s, s64, s32)
    assert torch.equal(s.cpu() == 0, s64 == 0) and torch.equal(s.cpu() == 1, s64 == 1)


def test_sorted_and_unsorted_edge_lists_take_their_routes_and_agree():
    """A list with ascending sources runs on its CSR offsets alone, any other on the by-source index; a stable sort by
    source keeps every node's order, so the two give the same bits."""
    from tgp import kernels as K
    x, ei, ew, batch = sparse_input("sizes")
    order = torch.sort(ei[0], stable=True).indices
    xd, eid, ewd, bd = _dev(x, ei, ew, batch)
    eis, ews = eid[:, order.to(DEV)].contiguous(), ewd[order.to(DEV)].contiguous()
    ptr = _ptr(batch).to(DEV)
    n = x.size(0)
    assert K.lapool_edge_group(eid, n).perm is not None and K.lapool_edge_group(eis, n).perm is None
    v0 = K.lapool_variation(xd, edge_index=eid, edge_weight=ewd)
    v1 = K.lapool_variation(xd, edge_index=eis, edge_weight=ews)
    assert torch.equal(v0, v1)
    l0 = K.lapool_leaders(v0, edge_index=eid, batch=bd, ptr=ptr)
    l1 = K.lapool_leaders(v1, edge_index=eis, batch=bd, ptr=ptr)
    assert torch.equal(l0.flags, l1.flags) and torch.equal(l0.col_of, l1.col_of)
    assert torch.equal(K.lapool_assign(xd, l0)[0], K.lapool_assign(xd, l1)[0])


def test_unbatched_pooler_is_one_pass_over_the_batch():
    from tgp.poolers import LaPooling
    x, ei, ew, batch = sparse_input("sizes")
    xd, eid, ewd, bd = _dev(x, ei, ew, batch)
    with torch.no_grad():
        out = LaPooling(batched=False)(x=xd, adj=eid, edge_weight=ewd, batch=bd)
    v, lead, s = R.select(x.double(), edge_index=ei, edge_weight=ew.double(), batch=batch)
    assert out.so.s.shape == (x.size(0), 70)
    if torch.equal(out.so.leader_mask.cpu(), lead):  # (a random input may hold a near-tie: values only for equal sets)
        torch.testing.assert_close(out.so.s.cpu().double(), s, rtol=1e-5, atol=1e-5)
    from tgp.select import LaPoolSelect
    one = LaPoolSelect(batched_representation=False)(xd[:1], eid[:, :0])  # one node, no edge
    assert torch.equal(one.s, torch.ones(1, 1, device=DEV))


# ---------------------------------------------------------------------------------- 5. ties and degenerate inputs
def test_ring_with_constant_features_makes_every_node_a_leader():
    from tgp.select import LaPoolSelect
    n = 70
    ring = torch.stack([torch.arange(n), (torch.arange(n) + 1) % n])
    ei = torch.cat([ring, ring.flip(0)], 1).to(DEV)
    x = torch.full((n, 5), 0.7, device=DEV)
    so = LaPoolSelect(batched_representation=False)(x, ei)
    assert bool(so.leader_mask.all()) and torch.equal(so.s, torch.eye(n, device=DEV))
    adj = torch.zeros(1, n, n, device=DEV)
    adj[0, ei[0], ei[1]] = 1.0
    so = LaPoolSelect()(x.unsqueeze(0), adj)
    assert bool(so.leader_mask.all()) and torch.equal(so.s, torch.eye(n, device=DEV).unsqueeze(0))


def test_zero_row_is_uniform_over_its_graphs_leaders():
    from tgp import kernels as K
    x = torch.randn(2, 9, 6, device=DEV)
    x[0, 4] = 0
    x[1, 7] = 0
    flags = torch.zeros(2, 9, dtype=torch.bool, device=DEV)
    flags[0, [0, 2, 8]] = True
    flags[1, [1, 3, 4, 5, 6]] = True
    s, _ = K.lapool_assign(x, K.lapool_columns(flags))
    assert s.shape == (2, 9, 5)
    assert torch.equal(s[0, 4], torch.tensor([1 / 3, 1 / 3, 1 / 3, 0, 0], device=DEV))
    assert torch.equal(s[1, 7], torch.full((5,), 0.2, device=DEV))


def test_one_graph_batch_and_run_to_run_bits():
    from tgp.select import LaPoolSelect
    x, ei, ew, batch = sparse_input("wide")
    keep = (batch[ei[0]] == 1)
    lo = int(_ptr(batch)[1])
    x1, ei1, ew1 = x[batch == 1].to(DEV), (ei[:, keep] - lo).to(DEV), ew[keep].to(DEV)
    sel = LaPoolSelect(batched_representation=False)
    a = sel(x1, ei1, ew1)
    b = sel(x1, ei1, ew1, batch=torch.zeros(x1.size(0), dtype=torch.long, device=DEV))
    assert torch.equal(a.s, b.s) and torch.equal(a.leader_mask, b.leader_mask)
    xd, eid, ewd, bd = _dev(x, ei, ew, batch)
    first = sel(xd, eid, ewd, batch=bd)
    for _ in range(3):
        again = sel(xd, eid, ewd, batch=bd)
        assert torch.equal(first.s, again.s)
    x3, a3, m3 = _dev(*dense_input("n37f5"))
    first = LaPoolSelect()(x3, a3, mask=m3)
    assert torch.equal(first.s, LaPoolSelect()(x3, a3, mask=m3).s)
    # a graph's result does not depend on its neighbours in the batch
    part = first.s[1:2]
    alone = LaPoolSelect()(x3[1:2], a3[1:2], mask=m3[1:2]).s
    assert torch.equal(part[..., :alone.size(-1)], alone)


# ------------------------------------------------------------------------------------------------------- 6. backward
def _pooled_sq(case, dtype):
    """sum(x_pool ** 2) of a fixture case through the restatement on the host; returns (the original x leaf, value)."""
    inp = case["inputs"]
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    ew = inp.get("edge_weight")
    ew = None if ew is None else ew.to(dtype)
    if inp.get("adj") is not None:
        _, _, s = R.select(x, inp["adj"].to(dtype), inp.get("mask"))
        return x, (torch.einsum("bnk,bnf->bkf", s, x) ** 2).sum()
    if case["cfg"].get("batched", True):
        xd, adj, mask = R.densify(x, inp["edge_index"], ew, inp.get("batch"))
        _, _, s = R.select(xd, adj, mask)
        return x, (torch.einsum("bnk,bnf->bkf", s, xd) ** 2).sum()
    batch = inp.get("batch")
    _, _, s = R.select(x, edge_index=inp["edge_index"], edge_weight=ew, batch=batch)
    total = 0
    for lo, hi in R._segments(x.size(0), batch):
        total = total + ((s[lo:hi].t() @ x[lo:hi]) ** 2).sum()
    return x, total


@pytest.mark.parametrize("name", sorted(CASES))
def test_backward_against_the_fixtures_float64_gradients(name):
    case = CASES[name]
    want = case["f64"]["grads"]["x"]
    x64, y64 = _pooled_sq(case, torch.float64)
    torch.testing.assert_close(torch.autograd.grad(y64, x64)[0], want, rtol=1e-9, atol=1e-9)  # the restatement's own
    x32, y32 = _pooled_sq(case, torch.float32)
    g32 = torch.autograd.grad(y32, x32)[0]
    x, out = _run_case(case, requires_grad=True)
    (g,) = torch.autograd.grad((out.x ** 2).sum(), x)
    _within(f"{name} dX", g, want, g32)


def _assign_paths(x, flags, mask=None, batch=None):
    from tgp import functions as Fn
    from tgp import kernels as K

    def kernel():
        xd = x.to(DEV).clone().requires_grad_(True)
        md, bd = _dev(mask, batch)
        lead = K.lapool_columns(flags.to(DEV), mask=md, batch=bd, ptr=None if batch is None else _ptr(batch).to(DEV))
        return {"s": Fn.lapool_assign(xd, lead)}, {"x": xd}

    def oracle(dtype):
        xc = x.to(dtype).clone().requires_grad_(True)
        return {"s": R.assign(xc, flags, mask=mask, batch=batch)}, {"x": xc}

    return kernel, oracle


@pytest.mark.parametrize("name", ["sizes", "wide"])
def test_assign_backward_sparse(name):
    x, ei, ew, batch = sparse_input(name)
    _, flags, _ = R.select(x.double(), edge_index=ei, edge_weight=ew.double(), batch=batch)
    kernel, oracle = _assign_paths(x, flags, batch=batch)
    check_grad_paths(f"lapool-{name}", kernel, oracle, ["x"])


@pytest.mark.parametrize("name", ["n37f5", "n64f64", "special"])
def test_assign_backward_dense(name):
    x, a, mask = dense_input(name)
    _, flags, _ = R.select(x.double(), a.double(), mask)
    kernel, oracle = _assign_paths(x, flags, mask=mask)
    check_grad_paths(f"lapool-{name}", kernel, oracle, ["x"])


def test_leader_and_padded_rows_of_ds_do_not_reach_dx():
    from tgp import functions as Fn
    from tgp import kernels as K
    x, a, mask = dense_input("n37f5")
    _, flags, _ = R.select(x.double(), a.double(), mask)
    xd, md, fd = _dev(x, mask, flags)
    grads = []
    up = torch.randn(3, 37, int(flags.sum(1).max()), device=DEV)
    for junk in (0.0, 1e3):
        leaf = xd.clone().requires_grad_(True)
        s = Fn.lapool_assign(leaf, K.lapool_columns(fd, mask=md))
        g = up.clone()
        g[fd | ~md] += junk * torch.randn_like(g[fd | ~md])
        grads.append(torch.autograd.grad(s, leaf, g)[0])
    assert bool((grads[0] != 0).any()) and torch.equal(grads[0], grads[1])
    assert torch.equal(grads[0][~md], torch.zeros_like(grads[0][~md]))


# --------------------------------------------------------------------------------------------------------- 7. memory
def test_selector_memory_stays_far_below_the_cross_graph_matrix():
    from tgp.select import LaPoolSelect
    g = torch.Generator().manual_seed(5)
    B, n, F = 64, 64, 16
    eis = []
    for b in range(B):
        up = torch.triu(torch.rand(n, n, generator=g) < 3.0 / n, 1)
        eis.append((up | up.t()).nonzero().t() + b * n)
    ei = torch.cat(eis, 1).to(DEV)
    x = torch.randn(B * n, F, generator=g).to(DEV)
    batch = torch.arange(B).repeat_interleave(n).to(DEV)
    sel = LaPoolSelect(batched_representation=False)
    assert bool((ei[0, 1:] >= ei[0, :-1]).all())  # the usual row-sorted layout
    so = sel(x, ei, batch=batch)  # (first call: library, pinned words, the batch's memoised facts)
    k_total = int(so.leader_mask.sum())
    assert k_total >= 512, k_total
    del so
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    so = sel(x, ei, batch=batch)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    composed = B * n * k_total * 4
    print(f"K_total {k_total}, K_max {so.s.size(1)}, growth {growth} bytes, composed matrix {composed} bytes")
    assert growth < composed / 4, (growth, composed)
