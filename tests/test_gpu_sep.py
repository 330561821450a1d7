"""SEP pooling on the device: the per-graph coding-tree kernel of csrc/sep_select.hip against the reference's stored
results (tests/golden/golden_sep_v1.pt) and against the restatement run in the kernel's arithmetic
(tests/sep_restatement.py, ``arith="kernel"``), the routes, the batch structure, determinism and the status word.

Exact labels are asked only of graphs that pass condition (c) of the fixture's generator: in the kernel-arithmetic run
every decision's gap to the best candidate with other inputs is at least 1e-9 of the largest term (the device's
logarithm may round differently from the host's by an ulp, 1e-16).  Seeds are walked until a graph passes; the last
test asserts that at most one seed in ten was skipped.  Unweighted graphs have integer volumes, and sparse ones are
full of candidates that are equal in exact arithmetic but computed from other inputs (2 ln 4 against 4 ln 2), which
(c) rightly drops; the unweighted graphs here are denser (about 16 neighbours), where volumes vary enough."""
import functools
import os

import pytest
import torch

import sep_restatement as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_sep_v1.pt"), weights_only=True)["cases"]
TOL = dict(rtol=1e-5, atol=1e-5)
GAP = 1e-9
TALLY = {"draws": 0, "skipped": 0}


def dev():
    return torch.device("cuda:0")


def limit():
    from tgp import kernels as K
    return K.sep_max_nodes()


def sizes():
    return [1, 2, 3, 5, 63, 64, 65, limit() - 1, limit()]  # tiny graphs, around a wave, at the LDS limit


def make_graph(n, seed, weighted):
    """Undirected, both directions listed: (edge_index, weight or None) on the host."""
    g = torch.Generator().manual_seed(seed)
    a = torch.triu(torch.rand(n, n, generator=g) < min(0.6, (6.0 if weighted else 16.0) / max(n, 1)), 1)
    ei = a.nonzero().t()
    ei = torch.cat([ei, ei.flip(0)], 1).contiguous()
    w = None
    if weighted:
        m = torch.rand(n, n, generator=g) + 0.1
        w = (m + m.t())[ei[0], ei[1]].contiguous()
    return ei, w


def restate(n, ei, w, batch=None, arith="kernel", gaps=None):
    lab, k = R.sep_select(n, ei.numpy(), None if w is None else w.numpy(), None if batch is None else batch.numpy(),
                          arith, gaps)
    return torch.from_numpy(lab), k


@functools.lru_cache(maxsize=None)
def usable_graphs(n, weighted, count=4):
    """``count`` graphs of ``n`` nodes that pass (c), with their labels in the kernel's arithmetic (computed once)."""
    out, seed = [], 1000 * n + (500 if weighted else 0)
    while len(out) < count:
        ei, w = make_graph(n, seed, weighted)
        gaps = {}
        lab, k = restate(n, ei, w, gaps=gaps)
        TALLY["draws"] += 1
        if gaps.get("min_ratio", float("inf")) >= GAP:
            out.append((ei, w, lab, k))
        else:
            TALLY["skipped"] += 1
        seed += 1
    return out


def join(graphs):
    """(edge_index, weight, batch, expected labels, expected count) of graphs given as (n, ei, w, labels, k)."""
    eis, ws, bs, labs, off, koff = [], [], [], [], 0, 0
    for gi, (n, ei, w, lab, k) in enumerate(graphs):
        eis.append(ei + off), ws.append(w), bs.append(torch.full((n,), gi, dtype=torch.long)), labs.append(lab + koff)
        off, koff = off + n, koff + k
    w = None if ws[0] is None else torch.cat(ws)
    return torch.cat(eis, 1).contiguous(), w, torch.cat(bs), torch.cat(labs), koff


def select(ei, w, batch, n=None, **kw):
    from tgp.select import sep_select
    d = dev()
    return sep_select(ei.to(d), None if w is None else w.to(d), None if batch is None else batch.to(d), n, **kw)


# ------------------------------------------------------------------------------------------------ fixture parity
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_gives_the_reference_labels_and_pooled_outputs(name):
    from tgp.poolers import SEPPooling
    c = CASES[name]
    i, want, d = c["inputs"], c["expected"], dev()
    x, ei = i["x"].to(d), i["edge_index"].to(d)
    ew = None if i["edge_weight"] is None else i["edge_weight"].to(d)
    batch = None if i["batch"] is None else i["batch"].to(d)
    pool = SEPPooling(**c["cfg"])
    out = pool(x=x, adj=ei, edge_weight=ew, batch=batch)
    assert out.so.__dict__["_sep_route"] == "native"
    assert out.so.num_supernodes == want["num_supernodes"]
    assert torch.equal(out.so.cluster_index.cpu(), want["cluster_index"])
    torch.testing.assert_close(out.x.cpu(), want["x"], **TOL)
    assert torch.equal(out.edge_index.cpu(), want["edge_index"])
    if want["edge_weight"] is None:  # (unweighted input, no normalisation: the reference returns no weights)
        assert out.edge_weight is None
    else:
        torch.testing.assert_close(out.edge_weight.cpu(), want["edge_weight"], **TOL)
    assert torch.equal(out.batch.cpu(), want["batch"]) if want["batch"] is not None else out.batch is None
    torch.testing.assert_close(pool(x=out.x, so=out.so, lifting=True).cpu(), want["x_lifted"], **TOL)


def test_hand_graphs_in_one_batch_exercise_the_id_tie_break():
    hand = [CASES[n] for n in sorted(CASES) if n.startswith("sep_hand_")]
    graphs = [(c["inputs"]["x"].size(0), c["inputs"]["edge_index"], None, c["expected"]["cluster_index"],
               c["expected"]["num_supernodes"]) for c in hand]
    ei, w, batch, want, k = join(graphs)
    so = select(ei, w, batch)
    assert so.num_supernodes == k and torch.equal(so.cluster_index.cpu(), want)


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("which", range(9))
def test_kernel_matches_the_restatement_in_its_arithmetic(which, weighted):
    n = sizes()[which]
    graphs = [(n,) + g for g in usable_graphs(n, weighted)]
    for part in (graphs[:1], graphs[1:4]):  # one graph (with a batch vector of one id), three graphs
        ei, w, batch, want, k = join(part)
        so = select(ei, w, batch, sum(g[0] for g in part))
        assert so.__dict__["_sep_route"] == "native"
        assert so.num_supernodes == k and torch.equal(so.cluster_index.cpu(), want), (n, weighted, len(part))
    ei, w, _, want, k = join(graphs[:1])
    so = select(ei, w, None, n)  # and without a batch vector
    assert so.num_supernodes == k and torch.equal(so.cluster_index.cpu(), want)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_forty_graphs_of_every_size_in_one_batch(weighted):
    graphs = [(n,) + g for n in sizes() for g in usable_graphs(n, weighted)]  # 36
    graphs += [(17,) + g for g in usable_graphs(17, weighted)]                # 40
    order = torch.randperm(len(graphs), generator=torch.Generator().manual_seed(5)).tolist()
    ei, w, batch, want, k = join([graphs[i] for i in order])
    so = select(ei, w, batch)
    assert so.__dict__["_sep_route"] == "native" and so.num_supernodes == k
    assert torch.equal(so.cluster_index.cpu(), want)


# ------------------------------------------------------------------------------------------------ routes
def test_graphs_over_the_limit_take_the_host_route_graph_by_graph():
    big_n = limit() + 1
    big_ei, big_w = make_graph(big_n, 77, True)
    big = select(big_ei, big_w, None, big_n, route="host")  # the host route alone
    small = [(20,) + g for g in usable_graphs(20, True)[:2]]
    graphs = [small[0], (big_n, big_ei, big_w, big.cluster_index.cpu(), big.num_supernodes), small[1]]
    ei, w, batch, want, k = join(graphs)
    so = select(ei, w, batch)
    assert so.__dict__["_sep_route"] == "mixed"
    assert so.num_supernodes == k and torch.equal(so.cluster_index.cpu(), want)
    so = select(big_ei, big_w, None, big_n)
    assert so.__dict__["_sep_route"] == "host" and torch.equal(so.cluster_index, big.cluster_index)
    with pytest.raises(ValueError, match="route='native'"):
        select(ei, w.double(), batch, route="native")


def test_float64_weights_and_an_unsorted_batch_take_the_host_route():
    (ei, w, lab, k), = usable_graphs(20, True)[:1]
    so = select(ei, w.double(), None, 20)
    assert so.__dict__["_sep_route"] == "host" and so.cluster_index.is_cuda
    g64 = {}
    want, _ = restate(20, ei, w, arith="f64", gaps=g64)
    assert g64["min_ratio"] >= 1e-5 and torch.equal(so.cluster_index.cpu(), want)
    batch = torch.tensor([1] * 10 + [0] * 10)
    keep = (batch[ei[0]] == batch[ei[1]])
    so = select(ei[:, keep], w[keep], batch)
    want, k = restate(20, ei[:, keep], w[keep], batch, arith="f64")
    assert so.__dict__["_sep_route"] == "host" and so.num_supernodes == k and torch.equal(so.cluster_index.cpu(), want)


# ------------------------------------------------------------------------------------------------ batch structure
def test_empty_graph_ids_edgeless_graphs_isolated_nodes_and_single_edges():
    (e1, w1, _, _), (e2, w2, _, _) = usable_graphs(20, True)[:2]
    iso = (e2[0] % 5 != 2) & (e2[1] % 5 != 2)  # every fifth node of the third graph loses its edges
    pairs = torch.arange(12).view(6, 2).t()  # six components of one edge each
    pairs = torch.cat([pairs, pairs.flip(0)], 1)
    ei = torch.cat([e1, e2[:, iso] + 27, pairs + 47], 1)  # graph 1 (7 nodes) has no edges, graph id 3 has no nodes
    w = torch.cat([w1, w2[iso], torch.ones(12)])
    batch = torch.tensor([0] * 20 + [1] * 7 + [2] * 20 + [4] * 12)
    gaps = {}
    want, k = restate(59, ei, w, batch, gaps=gaps)
    assert gaps.get("min_ratio", 1.0) >= GAP
    so = select(ei, w, batch)
    assert so.__dict__["_sep_route"] == "native" and so.num_supernodes == k
    assert torch.equal(so.cluster_index.cpu(), want)
    assert want[20:27].tolist() == list(range(int(want[20]), int(want[20]) + 7))  # the identity on the edgeless graph
    assert want[47:].tolist() == list(range(int(want[47]), int(want[47]) + 12))  # two singletons per single edge
    so = select(torch.zeros(2, 0, dtype=torch.long), None, batch)  # no edges at all
    assert so.cluster_index.cpu().tolist() == list(range(59))


# ------------------------------------------------------------------------------------------------ determinism
def test_same_bits_on_every_call_and_wherever_the_graph_stands():
    graphs = [(n,) + usable_graphs(n, True)[0] for n in (64, 20, 5, 65)]
    ei, w, batch, want, k = join(graphs)
    a, b = select(ei, w, batch), select(ei.clone(), w.clone(), batch.clone())
    assert torch.equal(a.cluster_index, b.cluster_index) and a.num_supernodes == b.num_supernodes == k
    probe = graphs[1]
    alone = select(probe[1], probe[2], None, probe[0]).cluster_index.cpu()
    for where in (0, 3):
        rest = [g for g in graphs if g is not probe]
        rest.insert(where, probe)
        ei, w, batch, _, _ = join(rest)
        got = select(ei, w, batch).cluster_index.cpu()[batch == where]
        assert torch.equal(got - got.min(), alone)  # (labels of a graph start at its first cluster: alone's are 0-based)


# ------------------------------------------------------------------------------------------------ status
def host_groups(idx, n):
    """CSR offsets and edge positions grouped by ``idx`` (stable), built on the host from a clean list."""
    order = torch.sort(idx, stable=True).indices.to(torch.int32)
    ptr = torch.zeros(n + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(torch.bincount(idx, minlength=n), 0).to(torch.int32)
    return ptr, order


def raw_select(clean_ei, ei, w, batch, num_graphs, sentinel=-7):
    """The C entry on hand-made inputs: the two edge-position indices come from ``clean_ei`` (so that an endpoint that
    is out of range in ``ei`` never reaches an index builder); (status, total, cluster_index pre-filled with sentinel)."""
    from tgp import _native as N
    d = dev()
    n, E = batch.numel(), ei.size(1)
    sp, so_ = host_groups(clean_ei[0], n)
    dp, do_ = host_groups(clean_ei[1], n)
    sp, so_, dp, do_ = sp.to(d), so_.to(d), dp.to(d), do_.to(d)
    src, dst, w = ei[0].contiguous().to(d), ei[1].contiguous().to(d), w.to(d)
    gid = batch.to(torch.int32).to(d)
    gptr = torch.zeros(num_graphs + 1, dtype=torch.int32)
    gptr[1:] = torch.cumsum(torch.bincount(batch, minlength=num_graphs), 0).to(torch.int32)
    gptr = gptr.to(d)
    out = torch.full((n,), sentinel, dtype=torch.int64, device=d)
    counts = torch.zeros(2, num_graphs, dtype=torch.int32, device=d)
    words = torch.zeros(2, dtype=torch.int32, device=d)
    rc = N.lib().tgp_sep_select_f32(N.ptr(sp), N.ptr(so_), N.ptr(dp), N.ptr(do_), N.ptr(src), N.ptr(dst), N.ptr(w),
                                    N.ptr(gid), N.ptr(gptr), n, E, num_graphs, 16, N.ptr(out), N.ptr(counts[0]),
                                    N.ptr(counts[1]), N.ptr(words), N.stream_ptr(d))
    assert rc == 0
    torch.cuda.synchronize()
    status, total = words.tolist()
    return status, total, out.cpu()


def test_refused_inputs_set_their_bit_and_leave_the_flagged_graph_unwritten():
    from tgp import kernels as K
    parts = [(n,) + usable_graphs(n, True)[0] for n in (5, 3, 5)]
    ei, w, batch, want, k = join(parts)
    n = batch.numel()
    st, total, clean = raw_select(ei, ei, w, batch, 3)
    assert st == 0 and total == k and torch.equal(clean, want)
    k0, k1 = parts[0][4], parts[1][4]
    at = int((batch[ei[0]] == 1).nonzero()[0])  # an edge of the middle graph (nodes 5, 6, 7)

    def flagged(status, total_, got, bit):
        assert status == bit and total_ == k - k1
        assert bool((got[5:8] == -7).all())  # the flagged graph is unwritten ...
        assert torch.equal(got[:5], clean[:5]) and torch.equal(got[8:], clean[8:] - k1)  # ... the others are complete

    bad = ei.clone()
    bad[1, at] = n + 5  # an endpoint >= N
    flagged(*raw_select(ei, bad, w, batch, 3), K.SEP_BAD_INPUT)
    bad[1, at] = -1
    flagged(*raw_select(ei, bad, w, batch, 3), K.SEP_BAD_INPUT)
    bad = ei.clone()
    bad[1, at] = 0  # an edge between two graphs (the in-edge index still lists it at its old destination)
    flagged(*raw_select(ei, bad, w, batch, 3), K.SEP_BAD_INPUT)
    neg = w.clone()
    neg[at] = -3.0
    flagged(*raw_select(ei, ei, neg, batch, 3), K.SEP_BAD_WEIGHT)
    nan = w.clone()
    nan[at] = float("nan")
    flagged(*raw_select(ei, ei, nan, batch, 3), K.SEP_BAD_WEIGHT)
    st, total, got = raw_select(ei, ei, w, torch.cat([batch, torch.full((17,), 3)]), 4)  # 17 nodes > max_n = 16
    assert st == K.SEP_OVER_LIMIT and total == k and torch.equal(got[:n], clean) and bool((got[n:] == -7).all())
    # through the wrapper (inputs whose endpoints are all in range: the index builders see them too)
    two = ei.clone()
    two[:, at] = torch.tensor([5, 0])
    with pytest.raises(ValueError, match="two graphs"):
        select(two, w, batch)
    with pytest.raises(ValueError, match="finite and non-negative"):
        select(ei, neg, batch)
    with pytest.raises(ValueError, match="finite and non-negative"):
        select(ei, nan, batch)
    assert k0 > 0


# ------------------------------------------------------------------------------------------------ the whole pooler
def test_whole_pooler_on_a_device_batch_fused_and_unfused_agree():
    from tgp.poolers import SEPPooling
    d = dev()
    graphs = [(n,) + g for n in (20, 17, 5) for g in usable_graphs(n, True)[:2]]
    ei, w, batch, want, k = join(graphs)
    order = torch.argsort(ei[0] * batch.numel() + ei[1])  # row-major sorted, the layout the fused launch takes
    ei, w, batch = ei[:, order].contiguous().to(d), w[order].to(d), batch.to(d)
    x = torch.randn(batch.numel(), 8, generator=torch.Generator().manual_seed(1)).to(d)
    pool = SEPPooling()
    out = pool(x=x, adj=ei, edge_weight=w, batch=batch)
    assert out.so.num_supernodes == k and torch.equal(out.so.cluster_index.cpu(), want)
    assert tuple(out.x.shape) == (k, 8) and out.batch.numel() == k
    firsts = torch.tensor([int(g[3].max()) + 1 for g in graphs])
    assert torch.equal(out.batch.cpu(), torch.repeat_interleave(torch.arange(len(graphs)), firsts))
    assert out.edge_index.size(0) == 2 and out.edge_weight.numel() == out.edge_index.size(1)
    assert int(out.edge_index.max()) < k and bool((out.edge_index[0] != out.edge_index[1]).all())
    assert pool.reduce_connect(x, ei, w, out.so, batch) is not None  # the forward above took the fused launch
    x2, b2 = pool.reduce(x=x, so=out.so, batch=batch)
    ei2, w2 = pool.connect(edge_index=ei, so=out.so, edge_weight=w, batch_pooled=b2)
    torch.testing.assert_close(out.x, x2, **TOL)
    assert torch.equal(out.batch, b2) and torch.equal(out.edge_index, ei2)
    torch.testing.assert_close(out.edge_weight, w2, **TOL)
    pre = pool.precoarsening(edge_index=ei, edge_weight=w, batch=batch, num_nodes=x.size(0))
    (multi,) = pool.multi_level_precoarsening(1, edge_index=ei, edge_weight=w, batch=batch, num_nodes=x.size(0))
    for got in (pre, multi):
        assert torch.equal(got.so.cluster_index, out.so.cluster_index) and torch.equal(got.edge_index, out.edge_index)
        torch.testing.assert_close(got.edge_weight, out.edge_weight, **TOL)
        assert torch.equal(got.batch, out.batch)
    lifted = pool(x=out.x, so=out.so, lifting=True)
    torch.testing.assert_close(lifted, out.x[out.so.cluster_index], **TOL)


# ------------------------------------------------------------------------------------------------ the seed walk
def test_at_most_one_seed_in_ten_was_skipped():
    for weighted in (False, True):
        for n in sizes() + [17, 20]:
            usable_graphs(n, weighted)  # (computed once; here only if this test runs alone)
    assert TALLY["draws"] >= 80 and 10 * TALLY["skipped"] <= TALLY["draws"], TALLY
