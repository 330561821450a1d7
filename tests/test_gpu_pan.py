"""PANConv / PANPooling on the device: parity with the fixture of the reference's pooler, the MET kernel against the
float64 restatement (pattern and order exact, values at fp32's own error), the score kernel against float64 with a bound
derived from the arithmetic, gradients one upstream path at a time (the helper of test_gpu_grad_paths.py), determinism,
memory, routing and memo hits, non-finite rows and the whole model."""
import math
import os

import pytest
import torch

import pan_restatement as R
from test_gpu_grad_paths import check_grad_paths

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_pan_v1.pt"), weights_only=True)["cases"]
TOL = dict(rtol=1e-5, atol=1e-5)
U = 2.0 ** -24  # fp32 unit roundoff


def dev():
    return torch.device("cuda:0")


def limit():
    from tgp import kernels
    return kernels.pan_max_graph_nodes()


def build(c, requires_grad=False):
    from tgp.nn import PANConv
    from tgp.poolers import PANPooling
    conv = PANConv(c["inputs"]["x"].size(1), c["cfg"]["in_channels"], c["filter_size"])
    conv.load_state_dict(c["conv"])
    p = PANPooling(**c["cfg"])
    p.load_state_dict(c["params"])
    conv, p = conv.to(dev()).eval(), p.to(dev()).eval()
    for q in list(conv.parameters()) + list(p.parameters()):
        q.requires_grad_(requires_grad)
    return conv, p


def on_dev(c):
    i = c["inputs"]
    return i["x"].to(dev()), i["edge_index"].to(dev()), None if i["batch"] is None else i["batch"].to(dev())


def ulp(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(v)) - 23) if v > 0 else 2.0 ** -149


# ------------------------------------------------------------------------------------------------ fixture parity
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_parity(name):
    from tgp import kernels
    c = CASES[name]
    e = c["expected"]
    conv, p = build(c)
    x, ei, batch = on_dev(c)
    with torch.no_grad():
        h, m = conv(x, ei, batch=batch)
        met = kernels.pan_record(m)
        assert met is not None and met.frame is not None, "device float32 inputs within the limit take the kernel"
        out = p(x=h, adj=m, batch=batch)
    assert torch.equal(m.indices().cpu(), e["met_index"])
    torch.testing.assert_close(m.values().cpu(), e["met_values"], **TOL)
    torch.testing.assert_close(h.cpu(), e["conv_out"], **TOL)
    so = out.so
    assert torch.equal(so.node_index.cpu(), e["so"]["node_index"])
    assert torch.equal(so.cluster_index.cpu(), e["so"]["cluster_index"])
    assert so.num_nodes == e["so"]["num_nodes"] and so.num_supernodes == e["so"]["num_supernodes"]
    torch.testing.assert_close(so.weight.cpu(), e["so"]["weight"], **TOL)
    torch.testing.assert_close(out.x.cpu(), e["x"], **TOL)
    if e["batch"] is None:
        assert out.batch is None
    else:
        assert torch.equal(out.batch.cpu(), e["batch"])
    assert out.edge_weight is None and out.edge_index.layout == torch.sparse_coo
    pooled = out.edge_index.coalesce()
    assert list(pooled.shape) == e["edge_index"]["size"]
    assert torch.equal(pooled.indices().cpu(), e["edge_index"]["indices"])
    torch.testing.assert_close(pooled.values().cpu(), e["edge_index"]["values"], **TOL)


# ------------------------------------------------------------------------------------------------ the MET kernel
def _random_graphs(sizes, deg, seed, directed=False):
    g = torch.Generator().manual_seed(seed)
    eis, bs, lo = [], [], 0
    for k, n in enumerate(sizes):
        m = int(n * deg) if n > 1 else 0
        ei = torch.randint(0, n, (2, m), generator=g)
        ei = ei[:, ei[0] != ei[1]]
        if not directed:
            ei = torch.cat([ei, ei.flip(0)], 1)
        eis.append(ei + lo)
        bs.append(torch.full((n,), k, dtype=torch.long))
        lo += n
    return torch.cat(eis, 1), torch.cat(bs), lo


def _shape(name):
    """(edge_index, batch or None, N, weight) of the named MET case, on the host."""
    lim = limit()
    w3 = torch.tensor([0.9, 0.6, -0.7, 0.45])
    single = {"n1": 1, "n2": 2, "n3": 3, "n63": 63, "n64": 64, "n65": 65, "limit_minus_1": lim - 1, "limit": lim,
              "limit_plus_1": lim + 1}
    if name in single:
        n = single[name]
        ei, _, _ = _random_graphs([n], 1.5, n)
        return ei, None, n, w3[:3] if n > 200 else w3
    if name == "edgeless":
        return torch.zeros(2, 0, dtype=torch.long), None, 5, w3
    if name == "isolated_nodes":
        ei, batch, n = _random_graphs([20, 33], 1.0, 5)
        keep = (ei[0] % 4 != 0) & (ei[1] % 4 != 0)  # every fourth node loses all its edges
        return ei[:, keep], batch, n, w3
    if name == "directed_path":
        return torch.stack([torch.arange(69), torch.arange(1, 70)]), None, 70, w3
    if name == "duplicates_and_loops":
        ei, batch, n = _random_graphs([17, 40], 1.5, 6, directed=True)
        loops = torch.arange(0, n, 3)
        return torch.cat([ei, ei[:, ::3], torch.stack([loops, loops]), ei[:, ::3]], 1), batch, n, w3
    if name == "unsorted_list":
        ei, batch, n = _random_graphs([30, 9, 51], 2.0, 7, directed=True)
        return ei[:, torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(8))], batch, n, w3
    if name == "unequal_batch":
        ei, batch, n = _random_graphs([1, 7, 64, 3, 130, 2, 65], 1.5, 9)
        return ei, batch, n, w3
    if name.startswith("L"):
        ei, batch, n = _random_graphs([24, 41], 1.2, 10, directed=True)
        return ei, batch, n, torch.tensor([0.8, -0.5, 0.7, 0.6, -0.9])[: int(name[1:]) + 1]
    raise KeyError(name)


MET_SHAPES = ["n1", "n2", "n3", "n63", "n64", "n65", "limit_minus_1", "limit", "limit_plus_1", "edgeless",
              "isolated_nodes", "directed_path", "duplicates_and_loops", "unsorted_list", "unequal_batch", "L0", "L1",
              "L2", "L3", "L4"]
_MET_REF = {}


def _met_reference(name):
    """The float64 restatement and the float32 one's error against it, computed once per shape."""
    if name not in _MET_REF:
        ei, batch, n, w = _shape(name)
        idx, v64 = R.met(ei, w.double(), n, batch)
        idx32, v32 = R.met(ei, w, n, batch)
        assert torch.equal(idx, idx32)
        _MET_REF[name] = (idx, v64, float((v32.double() - v64).abs().max()))
    return _MET_REF[name]


def _conv_for(w):
    from tgp.nn import PANConv
    conv = PANConv(2, 2, w.numel() - 1).to(dev())
    with torch.no_grad():
        conv.weight.copy_(w.to(dev()))
    return conv


@pytest.mark.parametrize("name", MET_SHAPES)
def test_met_kernel_against_the_float64_restatement(name):
    """Pattern and order exact; values within 4x the float32 restatement's own error on the same input, never below
    2 fp32 ulps of max|M| (the reciprocal square root may differ by one)."""
    ei, batch, n, w = _shape(name)
    idx, v64, own = _met_reference(name)
    conv = _conv_for(w)
    with torch.no_grad():
        met = conv.met(ei.to(dev()), n, None if batch is None else batch.to(dev()))
    native = name != "limit_plus_1"
    assert (met.frame is not None) == native, "one node past the limit routes to the composed form, the rest to the kernel"
    assert torch.equal(met.index.cpu(), idx)
    assert torch.equal(met.row_ptr.cpu().long(), torch.cat([torch.zeros(1, dtype=torch.long),
                                                            torch.cumsum(torch.bincount(idx[0], minlength=n), 0)]))
    err = float((met.values.double().cpu() - v64).abs().max())
    bound = max(4.0 * own, 2.0 * ulp(float(v64.abs().max())))
    print(f"met {name}: N={n} E={ei.size(1)} nnz={idx.size(1)} kernel err {err:.3e}, fp32 restatement err {own:.3e}, "
          f"bound {bound:.3e}")
    assert err <= bound
    if name == "edgeless":
        assert torch.equal(met.index.cpu(), torch.arange(n).repeat(2, 1))
        assert met.values.cpu().tolist() == [float(w[0])] * n


def test_met_composed_device_form_agrees_with_the_kernel():
    from tgp.nn import pan_met_composed
    ei, batch, n, w = _shape("unequal_batch")
    conv = _conv_for(w)
    with torch.no_grad():
        met = conv.met(ei.to(dev()), n, batch.to(dev()))
        idx, val = pan_met_composed(ei.to(dev()), conv.weight, n)
    assert met.frame is not None and torch.equal(idx, met.index)
    torch.testing.assert_close(val, met.values, rtol=1e-5, atol=1e-6)


def test_cross_graph_edges_and_unsorted_batches_take_the_composed_form():
    from tgp import kernels
    from tgp.utils.ops import batch_info
    ei, batch, n, w = _shape("unsorted_list")
    conv = _conv_for(w)
    cross = torch.cat([ei, torch.tensor([[3], [35]])], 1).to(dev())  # node 3 (graph 0) -> node 35 (graph 1)
    b = batch.to(dev())
    with torch.no_grad():
        met = conv.met(cross, n, b)
        assert met.frame is None, "the kernel declines an edge between two graphs"
        gptr = batch_info(b).memo["pan"][0]
        assert kernels.pan_route(cross, conv.weight, n, gptr, 51) == "composed"  # remembered for these graphs
        assert kernels.pan_route(cross, conv.weight, n, kernels.pan_one_graph_ptr(n, dev()), n) == "native"  # not for others
        idx, v64 = R.met(cross.cpu(), w.double(), n)  # (the whole input as one graph)
        assert torch.equal(met.index.cpu(), idx)
        torch.testing.assert_close(met.values.double().cpu(), v64, rtol=1e-5, atol=1e-6)
        # the same list without a batch vector is one graph of n nodes: native
        one = conv.met(cross, n, None)
        assert one.frame is not None and torch.equal(one.index.cpu(), idx)
        torch.testing.assert_close(one.values.double().cpu(), v64, rtol=1e-5, atol=1e-6)
        # a batch vector that is unsorted by construction (the first two nodes swap graphs): composed, over the whole input
        unsorted = b.clone()
        unsorted[0], unsorted[1] = 2, 0
        assert bool((unsorted[1:] < unsorted[:-1]).any())
        got = conv.met(ei.to(dev()), n, unsorted)
        idx_u, v64_u = R.met(ei, w.double(), n)
        assert got.frame is None and torch.equal(got.index.cpu(), idx_u)
        torch.testing.assert_close(got.values.double().cpu(), v64_u, rtol=1e-5, atol=1e-6)
        # float64 weights
        assert conv.double().met(ei.to(dev()), n, b).values.dtype == torch.float64
    bad = torch.cat([ei, torch.tensor([[2], [n + 5]])], 1).to(dev())
    with pytest.raises(IndexError, match="outside its table"):
        _conv_for(w).met(bad, n, b)


CROSS_CASES = {
    # the source is alone in its graph: its only column is masked from the start, the reach walk never looks at its edges
    "single_node_source": ([0, 1, 1], [[0], [1]]),
    # the source's earlier edges already reach every other node of its graph: the walk leaves before the crossing edge
    "earlier_edges_reach_all": ([0, 0, 0, 1, 1], [[0, 0, 1, 2, 0, 3], [1, 2, 0, 0, 3, 4]]),
    # ... and the crossing edge as the source's last one while the row's own walk has nothing left to add
    "last_edge_of_a_full_row": ([0, 0, 1, 1, 1], [[0, 1, 0, 2, 3], [1, 0, 3, 3, 4]]),
}


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("name", sorted(CROSS_CASES))
def test_every_cross_graph_edge_is_seen_by_the_count(name, L):
    """An edge between two graphs that the reach walk does not visit must still decline the kernel: the result is the
    composed form's, which is the definition on the whole input (the entry the edge creates is stored)."""
    batch, ei = (torch.tensor(v) for v in CROSS_CASES[name])
    n = batch.numel()
    w = torch.tensor([0.9, 0.6, -0.7, 0.45])[: L + 1]
    conv = _conv_for(w)
    with torch.no_grad():
        met = conv.met(ei.to(dev()), n, batch.to(dev()))
    idx, v64 = R.met(ei, w.double(), n)  # (the whole input as one graph)
    assert met.frame is None, "the kernel must decline"
    assert torch.equal(met.index.cpu(), idx)
    torch.testing.assert_close(met.values.double().cpu(), v64, rtol=1e-5, atol=1e-6)
    cross = (batch[ei[0]] != batch[ei[1]]).nonzero().view(-1)
    assert cross.numel() == 1
    s, d = int(ei[0, cross[0]]), int(ei[1, cross[0]])
    assert bool(((idx[0] == d) & (idx[1] == s)).any()), "the entry (target, source) of the crossing edge is stored"


@pytest.mark.parametrize("name", sorted(CROSS_CASES))
def test_an_out_of_range_endpoint_on_an_unvisited_edge_raises(name):
    batch, ei = (torch.tensor(v) for v in CROSS_CASES[name])
    n = batch.numel()
    cross = int((batch[ei[0]] != batch[ei[1]]).nonzero().view(-1)[0])
    bad = ei.clone()
    bad[1, cross] = n + 3  # the edge the reach walk does not visit now points outside [0, N)
    conv = _conv_for(torch.tensor([0.9, 0.6, -0.7]))
    with pytest.raises(IndexError, match="outside its table"):
        conv.met(bad.to(dev()), n, batch.to(dev()))
    neg = ei.clone()
    neg[1, cross] = -1
    with pytest.raises(IndexError, match="outside its table"):
        conv.met(neg.to(dev()), n, batch.to(dev()))


def test_met_is_deterministic():
    ei, batch, n, w = _shape("unequal_batch")
    conv = _conv_for(w)
    e, b = ei.to(dev()), batch.to(dev())
    with torch.no_grad():
        a, c = conv.met(e, n, b), conv.met(e, n, b)
    assert torch.equal(a.index, c.index) and torch.equal(a.values, c.values) and torch.equal(a.dinv, c.dinv)
    g = torch.randn(a.values.numel(), device=dev())
    from tgp import kernels
    assert torch.equal(kernels.pan_met_bwd(a, g), kernels.pan_met_bwd(a, g))


def test_met_memory_stays_below_the_composed_form():
    """A warm kernel call allocates M, the offsets and a scan workspace; the composed form also holds the L + 1 partial
    lists, their keys and the expansion of every product."""
    from tgp.nn import pan_met_composed
    ei, batch, n = _random_graphs([50] * 256, 2.0, 11)
    w = torch.tensor([0.9, 0.6, 0.7, 0.45])
    conv = _conv_for(w)
    e, b = ei.to(dev()), batch.to(dev())
    rises = {}
    with torch.no_grad():
        for who, call in (("kernel", lambda: conv.met(e, n, b)), ("composed", lambda: pan_met_composed(e, conv.weight, n))):
            call()  # warm: the memos, the workspace pools
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = call()
            torch.cuda.synchronize()
            rises[who] = torch.cuda.max_memory_allocated() - base
            del out
    nnz = int(conv.met(e, n, b).index.size(1))
    print(f"met warm call, 256 x 50 nodes, nnz {nnz}: peak rise kernel {rises['kernel']} bytes, composed {rises['composed']}")
    assert rises["kernel"] < rises["composed"]
    assert rises["kernel"] < 2 * (20 * nnz + 8 * n) + (1 << 20)  # M itself (16 + 4 bytes an entry), offsets, dinv: no L + 1 lists


# ------------------------------------------------------------------------------------------------ the score kernel
@pytest.mark.parametrize("use_tanh", [True, False], ids=["tanh", "identity"])
@pytest.mark.parametrize("f", [1, 16, 37])
def test_score_kernel_against_float64(f, use_tanh):
    """Any summation order of n terms is within (n - 1) u of the exact sum of the magnitudes: the bound per node is
    (F + column entries + 4) u (|beta0| sum|x p| + |beta1| sum|M_e|), times the activation's slope of at most 1, plus
    8 u for tanhf itself (within 2 ulp of a value below 1) and the store."""
    from tgp import kernels
    ei, batch, n, w = _shape("unequal_batch")
    conv = _conv_for(w)
    g = torch.Generator().manual_seed(f)
    x, p, beta = torch.randn(n, f, generator=g), torch.randn(f, generator=g), torch.tensor([0.7, -1.3])
    with torch.no_grad():
        met = conv.met(ei.to(dev()), n, batch.to(dev()))
        got, dot, colsum = kernels.pan_score(x.to(dev()), p.to(dev()), beta.to(dev()), met.col_group, met.values,
                                             use_tanh, want_terms=True)
        assert torch.equal(got, kernels.pan_score(x.to(dev()), p.to(dev()), beta.to(dev()), met.col_group, met.values,
                                                  use_tanh))
    idx, val = met.index.cpu(), met.values.double().cpu()
    t = R.raw_score(x.double(), idx, val, p.double(), beta.double())
    mag = beta[0].abs().double() * (x.double().abs() @ p.double().abs()) + beta[1].abs().double() * torch.zeros(
        n, dtype=torch.float64).index_add(0, idx[1], val.abs())
    count = torch.bincount(idx[1], minlength=n)
    bound = (f + count + 4).double() * U * mag + 8 * U
    want = torch.tanh(t) if use_tanh else t
    err = (got.double().cpu() - want).abs()
    print(f"pan_score f={f} tanh={use_tanh}: max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    torch.testing.assert_close(dot.double().cpu(), x.double() @ p.double(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(colsum.double().cpu(), torch.zeros(n, dtype=torch.float64).index_add(0, idx[1], val),
                               rtol=1e-5, atol=1e-5)


def test_selection_order_on_separated_scores():
    """The device route lists the kept nodes in the float64 restatement's order.  The scores are a shuffled grid
    (neighbours 3 / (N - 1) apart in the first feature, far beyond fp32's error) nudged by the column sums of M."""
    from tgp.poolers import PANPooling
    c = CASES["pan_undirected_batch"]
    conv, _ = build(c)
    _, ei, batch = on_dev(c)
    i = c["inputs"]
    n = i["x"].size(0)
    gen = torch.Generator().manual_seed(5)
    h = torch.zeros(n, 4)
    h[:, 0] = torch.linspace(-1.5, 1.5, n)[torch.randperm(n, generator=gen)]
    h[:, 1:] = torch.randn(n, 3, generator=gen)
    p = PANPooling(4, ratio=0.5).to(dev()).eval()
    with torch.no_grad():
        p.p.copy_(torch.tensor([1.0, 0.0, 0.0, 0.0]))
        p.beta.copy_(torch.tensor([1.0, 1e-3]))
        _, m = conv(i["x"].to(dev()), ei, batch=batch)
        out = p(x=h.to(dev()), adj=m, batch=batch)
    idx, val = R.met(i["edge_index"], c["conv"]["weight"].double(), n, i["batch"])
    _, score, perm, _, _, _, _ = R.pool(h.double(), idx, val, i["batch"], p.p.detach().double().cpu(),
                                        p.beta.detach().double().cpu())
    s = torch.sort(score).values
    assert float((s[1:] - s[:-1]).min()) >= 1e-4, "the construction no longer separates the scores"
    got = torch.empty_like(out.so.node_index)
    got[out.so.cluster_index] = out.so.node_index
    assert torch.equal(got.cpu(), perm)
    torch.testing.assert_close(out.so.weight.cpu().double(), score[out.so.node_index.cpu()], rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("zero_weight", [False, True], ids=["weights", "one_weight_zero"])
@pytest.mark.parametrize("name", ["pan_undirected_batch", "pan_directed_batch", "pan_identity", "pan_filter_4"])
def test_gradients_one_path_at_a_time(name, zero_weight):
    """The convolution's output alone, M's values alone, so.weight alone, x_pool alone and the fixture's objective, to
    x, lin, weight, p and beta, against float64 autograd of the restatement with the float32 restatement as the measure
    of fp32's own error.  ``one_weight_zero``: weight[1] = 0 (the cumulative product's gradient must not divide by it)."""
    c = CASES[name]
    i = c["inputs"]
    cw = c["conv"]["weight"].clone()
    if zero_weight:
        cw[1] = 0.0
    node_index, order = c["expected"]["so"]["node_index"], c["expected"]["so"]["cluster_index"]
    perm = torch.empty_like(node_index)
    perm[order] = node_index
    leaves = ["x", "weight", "lin.weight", "lin.bias", "p", "beta"]

    def kernel():
        conv, p = build(c, requires_grad=True)
        with torch.no_grad():
            conv.weight.copy_(cw.to(dev()))
        x, ei, batch = on_dev(c)
        x.requires_grad_(True)
        h, m = conv(x, ei, batch=batch)
        out = {"conv_out": h, "met_values": m.values()}
        if not zero_weight:  # (the stored selection belongs to the stored weights)
            res = p(x=h, adj=m, batch=batch)
            got = torch.empty_like(res.so.node_index)
            got[res.so.cluster_index] = res.so.node_index
            assert torch.equal(got.cpu(), perm)
            w = torch.zeros_like(res.so.weight).index_put((res.so.cluster_index,), res.so.weight)
            out.update(weight=w, x_pool=res.x, sum_sq=(res.x ** 2).sum())
        else:
            from tgp import functions, kernels
            met = kernels.pan_record(m)
            out["score"] = functions.pan_score(h, p.p, p.beta, met, True)
        lv = {"x": x, "weight": conv.weight, "lin.weight": conv.lin.weight, "lin.bias": conv.lin.bias, "p": p.p,
              "beta": p.beta}
        return out, lv

    def oracle(dtype):
        lv = {"x": i["x"].to(dtype), "weight": cw.to(dtype), "lin.weight": c["conv"]["lin.weight"].to(dtype),
              "lin.bias": c["conv"]["lin.bias"].to(dtype), "p": c["params"]["p"].to(dtype),
              "beta": c["params"]["beta"].to(dtype)}
        lv = {k: v.clone().requires_grad_(True) for k, v in lv.items()}
        h, idx, val = R.conv(lv["x"], i["edge_index"], lv["weight"], lv["lin.weight"], lv["lin.bias"], i["batch"])
        out = {"conv_out": h, "met_values": val}
        if not zero_weight:
            cfg = c["cfg"]
            _, _, _, weight, x_pool, _, _ = R.pool(h, idx, val, i["batch"], lv["p"], lv["beta"],
                                                   cfg.get("nonlinearity", "tanh"), perm=perm)
            out.update(weight=weight, x_pool=x_pool, sum_sq=(x_pool ** 2).sum())
        else:
            out["score"] = torch.tanh(R.raw_score(h, idx, val, lv["p"], lv["beta"]))
        return out, lv

    check_grad_paths(f"{name}/{zero_weight}", kernel, oracle, leaves)


# ------------------------------------------------------------------------------------------------ routing and memos
def test_pooling_reuses_what_the_convolution_knew(monkeypatch):
    from tgp import kernels
    c = CASES["pan_undirected_batch"]
    conv, p = build(c)
    x, ei, batch = on_dev(c)
    built = []
    real = kernels.edge_group
    monkeypatch.setattr(kernels, "edge_group", lambda *a, **k: built.append(1) or real(*a, **k))
    offsets = []
    real_off = kernels.csr_offsets
    monkeypatch.setattr(kernels, "csr_offsets", lambda *a, **k: offsets.append(1) or real_off(*a, **k))
    with torch.no_grad():
        h, m = conv(x, ei, batch=batch)
        met = kernels.pan_record(m)
        assert met is not None and met.row_ptr is not None and met._col_group is None
        p(x=h, adj=m, batch=batch)
        assert built == [1] and offsets == [] and met._col_group is not None  # the group index: built once, by the score
        p(x=h, adj=m, batch=batch)
        assert built == [1] and offsets == []  # the second pooling of the same M builds nothing
        # an M that did not come from PANConv: offsets and group index are built, and remembered for that tensor
        other = torch.sparse_coo_tensor(m.indices().clone(), m.values().clone(), m.shape).coalesce()
        out1 = p(x=h, adj=other, batch=batch)
        assert built == [1, 1] and offsets == [1]
        out2 = p(x=h, adj=other, batch=batch)
        assert built == [1, 1] and offsets == [1]
        assert torch.equal(out1.x, out2.x)
        # CSR in, CSR out
        out3 = p(x=h, adj=other.to_sparse_csr(), batch=batch)
        assert out3.edge_index.layout == torch.sparse_csr and torch.equal(out3.x, out1.x)
    # min_score and a callable activation take the composed score on the device and agree with the kernel's
    from tgp.poolers import PANPooling
    q = PANPooling(c["cfg"]["in_channels"], nonlinearity=torch.tanh).to(dev()).eval()
    q.load_state_dict(c["params"])
    assert q.selector._fused_act is None
    with torch.no_grad():
        out4 = q(x=h, adj=m, batch=batch)
    assert torch.equal(out4.so.node_index, out1.so.node_index)
    torch.testing.assert_close(out4.x, out1.x, **TOL)


def test_non_finite_rows_give_the_composed_forms_nan_mask():
    from tgp import functions, kernels
    c = CASES["pan_directed_batch"]
    conv, p = build(c)
    x, ei, batch = on_dev(c)
    x = x.clone()
    x[3] = float("nan")
    x[17, 1] = float("inf")
    x[30, 0] = float("-inf")
    with torch.no_grad():
        h, m = conv(x, ei, batch=batch)
        met = kernels.pan_record(m)
        agg = torch.zeros_like(x).index_add(0, met.index[0], met.values.view(-1, 1) * x[met.index[1]])
        want_h = torch.nn.functional.linear(agg, conv.lin.weight, conv.lin.bias)
        assert torch.equal(torch.isnan(h), torch.isnan(want_h)) and torch.equal(torch.isinf(h), torch.isinf(want_h))
        got = functions.pan_score(h, p.p, p.beta, met, True)
        want = torch.tanh(R.raw_score(h, met.index, met.values, p.p, p.beta))
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(got).any())
    ok = ~torch.isnan(want)
    torch.testing.assert_close(got[ok], want[ok], **TOL)


# ------------------------------------------------------------------------------------------------ the whole model
def test_whole_model_conv_pool_lift_trains():
    from tgp.nn import PANConv
    from tgp.poolers import PANPooling
    ei, batch, n = _random_graphs([30, 45, 12, 64], 1.5, 12)
    x = torch.randn(n, 8, generator=torch.Generator().manual_seed(3)).to(dev())
    ei, batch = ei.to(dev()), batch.to(dev())
    conv1, pool, conv2 = PANConv(8, 16, 3).to(dev()), PANPooling(16, ratio=0.5).to(dev()), PANConv(16, 4, 2).to(dev())
    h, m = conv1(x, ei, batch=batch)
    out = pool(x=torch.relu(h), adj=m, batch=batch)
    assert out.edge_index.layout == torch.sparse_coo and out.edge_weight is None
    assert out.x.shape == (out.so.num_supernodes, 16) and out.batch.numel() == out.so.num_supernodes
    h2, _ = conv2(out.x, out.edge_index, batch=out.batch)
    lifted = pool(x=h2, so=out.so, lifting=True)
    assert lifted.shape == (n, 4)
    lifted.pow(2).sum().backward()
    for mod in (conv1, pool, conv2):
        for name, q in mod.named_parameters():
            assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name
    assert float(conv1.weight.grad.abs().sum()) > 0 and float(pool.p.grad.abs().sum()) > 0
    assert float(pool.beta.grad.abs().sum()) > 0
