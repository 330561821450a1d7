"""Warm-state sequences: an operator is driven through cold call -> warm call -> in-place change -> call again on the SAME
tensor objects (tests/warm_state.py), every result held against the staged operators bit for bit and against the float64
CPU restatement, and every step asserts the memo hit or miss it was written to produce.  Then the per-(device, stream)
state: the epoch wrap, a state replaced under a pending prefetch, two interleaved streams.

Tolerances are the project's (FACTOR, FLOOR, CAP of tests/test_gpu_grad_paths.py); seeds are named where data is drawn."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warm_state as WS  # noqa: E402
from fuzz_compare import F64_BOUND  # noqa: E402
from warm_state import Step, run_sequence  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _cold_start():
    """Every test starts with nothing remembered (a fact left by another test must not decide a route here)."""
    import tgp
    tgp.clear_memos()
    yield


def _spy(monkeypatch, module, name, log, note=lambda result: result is not None):
    """Record what every call of ``module.name`` returned (``note(result)``) in ``log``; the function runs as it is."""
    real = getattr(module, name)

    def wrapped(*a, **k):
        out = real(*a, **k)
        log.append(note(out))
        return out

    monkeypatch.setattr(module, name, wrapped)


# ================================================================================== 1. one-launch sparse pooling
def _make_pooler(alias, f, dev):
    from tgp.poolers import get_pooler
    torch.manual_seed(17)  # the TopK projection: a fixed problem
    return (get_pooler("topk", in_channels=f, ratio=0.5) if alias == "topk" else get_pooler("graclus")).to(dev).eval()


def _pooled(pooler, x, ei, ew, batch):
    with torch.no_grad():
        out = pooler(x=x, adj=ei, edge_weight=ew, batch=batch)
    so = out.so
    return {"x": out.x, "batch": out.batch, "edge_index": out.edge_index, "edge_weight": out.edge_weight,
            "node_index": so.node_index, "cluster_index": so.cluster_index,
            "so_weight": None if so.weight is None else so.weight.detach(), "_so": so}


def _staged_on_clones(alias, pooler, x, ei, ew, batch):
    """The staged operators (Select, BaseReduce, SparseConnect) on clones: what ``sparse_pool_small`` documents itself
    bit-identical to."""
    xc, eic, ewc, bc = x.clone(), ei.clone(), ew.clone(), batch.clone()
    with torch.no_grad():
        so = (pooler.selector(x=xc, batch=bc) if alias == "topk" else
              pooler.selector(edge_index=eic, edge_weight=ewc, num_nodes=xc.size(0), batch=bc))
        xp, bp = pooler.reducer(xc, so, batch=bc)
        pe, pw = pooler.connector(eic, so, edge_weight=ewc, batch_pooled=bp)
    return {"x": xp, "batch": bp, "edge_index": pe, "edge_weight": pw, "node_index": so.node_index,
            "cluster_index": so.cluster_index, "so_weight": None if so.weight is None else so.weight.detach(), "_so": so}


def _sps_reference(alias, pooler, x, ei, ew, batch):
    cold = _staged_on_clones(alias, pooler, x, ei, ew, batch)
    so = cold["_so"]
    w = torch.ones(so.node_index.numel()) if so.weight is None else so.weight.detach().cpu()
    fields = (so.node_index.cpu(), so.cluster_index.cpu(), w, int(so.num_supernodes))
    r64, r32 = WS.pool_given_selection(alias, x.cpu(), ei.cpu(), ew.cpu(), batch.cpu(), fields)
    exact = ["batch", "edge_index"]
    # a cluster whose two nodes lie in two graphs (the moved boundary under Graclus): the reference's scatter leaves
    # either graph id, so the pooled batch vector has no single reference; it is held to the staged operators alone
    b, c = batch.cpu(), so.cluster_index.cpu()
    lo = torch.full((fields[3],), 1 << 40).scatter_reduce(0, c, b[fields[0]], "amin")
    hi = torch.full((fields[3],), -1).scatter_reduce(0, c, b[fields[0]], "amax")
    if bool((lo != hi).any()):
        for r in (r64, r32):
            del r["batch"]
        exact.remove("batch")
    return {"cold": cold, "bitwise": ["x", "batch", "edge_index", "edge_weight", "node_index", "cluster_index", "so_weight"],
            "r64": r64, "r32": r32, "exact": exact}


def _sps_sequence(alias, dev, give_ptrs, case, hits, seed=101):
    """(steps, call, reference, live tensors) of item 1 on one stream; ``hits``: what the spy on ``_edge_ptr_memo``
    records (cleared at the start of every call)."""
    from tgp import kernels as K
    from tgp.utils import ops
    x, ei_a, ei_b, ew, batch0, moved = (t.to(dev) for t in WS.sps_data(seed))
    ei, batch = ei_a.clone(), batch0.clone()
    pooler = _make_pooler(alias, x.size(1), dev)

    def call():
        hits.clear()
        return _pooled(pooler, x, ei, ew, batch)

    def ptr():
        return ops.batch_info(batch).ptr

    def ranges_remembered(yes):
        if not give_ptrs:
            assert K._EDGE_RANGES.get(ei, ptr()) is None
            return
        table = K._EDGE_RANGES.get(ei, ptr())
        assert (table is not None) == yes, (case, "edge ranges remembered", table is not None, "expected", yes)
        if yes:  # the ranges of the list as it is NOW
            assert torch.equal(table, torch.searchsorted(ei[0].contiguous(), ptr()))

    def after_cold(got):
        assert not any(hits), (case, "a new list must not be handed remembered ranges", hits)
        assert not K.sparse_pool_small_declined(ei)
        ranges_remembered(True)

    def after_warm(got):
        if give_ptrs:
            assert hits and all(hits), (case, "the warm call must be handed the remembered ranges", hits)
            if alias == "topk":  # mode 0 takes both tables
                assert got["_so"].__dict__.get("_assign_ptr") is not None
        else:
            assert not hits
        assert not K.sparse_pool_small_declined(ei)

    def after_refused(got):
        assert K.sparse_pool_small_declined(ei), (case, "an edge between two graphs must be refused")
        assert K._EDGE_RANGES.get(ei, ptr()) is None  # what a refused call searched for is forgotten again

    steps = [
        Step("cold", after=after_cold),
        Step("warm", before=lambda: ranges_remembered(True), after=after_warm),
        Step("other-list", change=lambda: ei.copy_(ei_b), before=lambda: ranges_remembered(False), after=after_cold),
        Step("moved-boundary", change=lambda: batch.copy_(moved),
             before=lambda: _assert(ops._INFO_OF_BATCH.get(batch) is None, "batch facts survived copy_"),
             after=after_refused),
        Step("list-back", change=lambda: ei.copy_(ei_a),
             before=lambda: _assert(not K.sparse_pool_small_declined(ei), "the refusal outlived the version"),
             after=after_refused),  # (list A has an edge across the moved boundary too)
        # the refusal is remembered for the LIST alone: with the batch vector back it costs the staged route, not a result
        Step("boundary-back", change=lambda: batch.copy_(batch0),
             before=lambda: _assert(K.sparse_pool_small_declined(ei), "the refusal is keyed on the list")),
        Step("list-again", change=lambda: ei.copy_(ei_a),
             before=lambda: _assert(not K.sparse_pool_small_declined(ei), "the refusal outlived the version"),
             after=after_cold),
        Step("warm-again", before=lambda: ranges_remembered(True), after=after_warm),
    ]
    return steps, call, (lambda: _sps_reference(alias, pooler, x, ei, ew, batch)), (x, ei, ew, batch)


def _assert(ok, what):
    assert ok, what


@pytest.mark.parametrize("switch", ["default", "no_ptrs", "no_arena"])
@pytest.mark.parametrize("alias", ["topk", "graclus"])
def test_one_launch_sparse_pooling_sequence(dev, alias, switch, monkeypatch):
    """Item 1: ``sparse_pool_small`` through the TopK (mode 0) and Graclus (mode 1) poolers in eval, 5 sorted graphs of 3
    to 64 nodes, F = 5 (seed 101).  Cold -> warm (the kernel is handed ``eptr``, mode 0 also ``assign_ptr``) -> another
    row-sorted list of the same E copied in -> a graph boundary moved so that an edge joins two graphs (refused: the
    staged operators run) -> the list copied back (the refusal must not outlive the version) -> ... ; every result equals
    the staged operators on clones bit for bit and the oracle within the project's bounds.  Finally the same list with a
    second ``graph_ptr`` object must not read the first one's ranges."""
    from tgp import kernels as K
    if switch == "no_ptrs":
        monkeypatch.setattr(K, "_SPS_GIVE_PTRS", False)
    if switch == "no_arena":
        monkeypatch.setattr(K, "_SPS_ARENA", False)
    case = f"sps_{alias}_{switch}"
    hits = []
    _spy(monkeypatch, K, "_edge_ptr_memo", hits)
    steps, call, reference, (x, ei, ew, batch) = _sps_sequence(alias, dev, switch != "no_ptrs", case, hits)
    run_sequence(steps, call, reference, case)
    # the same edge_index object, a second graph_ptr object of other contents
    from tgp.utils import ops
    ptr1 = ops.batch_info(batch).ptr
    ptr2 = torch.tensor([0, 10, 50, 100, 120, x.size(0)], device=dev)
    row = ei[0].contiguous()
    t2 = K.graph_edge_ptr(ei, ptr2)
    assert torch.equal(t2, torch.searchsorted(row, ptr2)) and not torch.equal(t2, torch.searchsorted(row, ptr1))
    assert K._EDGE_RANGES.get(ei, ptr1) is None and K._EDGE_RANGES.get(ei, ptr2) is t2
    assert torch.equal(K.graph_edge_ptr(ei, ptr1), torch.searchsorted(row, ptr1))


# ================================================================================================ 2. coalesce ladder
OPS = ["sum", "mean", "min", "max", "mul"]


def _coalesce_ref(ei, w, cl, k, op):
    def run(dtype):
        ww = torch.ones(ei.size(1), dtype=dtype) if w is None else w.cpu().to(dtype)
        rei, rw = WS._dense_ref_coalesce(ei.cpu(), ww, cl.cpu(), k, op, True)
        out = {"edge_index": rei}
        if w is not None:
            out["edge_weight"] = rw
        return out
    return WS.both(run)


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("op", OPS)
def test_coalesce_ladder_sequence(dev, op, weighted, monkeypatch):
    """Item 2: n = 200, E = 1500, supernode row 0 with 1100 raw entries (beyond the 1024 of ``_coalesce_rows``), seed 7.
    Auto route: the -5 retry sets ``_HUB_LISTS``; warm: the huge-row kernels are asked for at once (one attempt); an
    unsorted list without a hub copied in: the row-local route declines, ``_SORTED_ROWS`` says False, the general route
    runs; sorted in place: row-local again.  Against ``_dense_ref_coalesce`` in float64, indices exact."""
    from tgp import kernels as K
    ei_h, ei_u, ei_s, cl_hub, cl_flat, w, k = WS.hub_data(7)
    ei_h, ei_u, ei_s, cl, w = ei_h.to(dev), ei_u.to(dev), ei_s.to(dev), cl_hub.to(dev), (w.to(dev) if weighted else None)
    ei = ei_h.clone()
    index = K.build_assign_index(cl, k)
    rows, general = [], []
    _spy(monkeypatch, K, "_coalesce_rows", rows, note=lambda r: r if isinstance(r, int) else "out")
    _spy(monkeypatch, K, "_coalesce_general", general)
    counts = []
    _spy(monkeypatch, K, "_count_fill", counts, note=lambda r: r if isinstance(r, int) else "out")

    def call():
        del rows[:], general[:], counts[:]
        pe, pw = K.coalesce_edges(ei, w, cl, k, op, True, assign_index=index)
        return {"edge_index": pe, "edge_weight": pw}

    def reference():
        eic, wc = ei.clone(), (None if w is None else w.clone())
        pe, pw = K.coalesce_edges(eic, wc, cl, k, op, True, assign_index=index)
        r64, r32 = _coalesce_ref(ei, w, cl, k, op)
        return {"cold": {"edge_index": pe, "edge_weight": pw}, "bitwise": ["edge_index", "edge_weight"],
                "r64": r64, "r32": r32, "exact": ["edge_index"]}

    def after_retry(got):
        assert rows == ["out"] and counts == [-5, "out"] and not general, (rows, counts, general)
        assert K._HUB_LISTS.get(ei) is not None

    def after_hub_warm(got):
        assert rows == ["out"] and counts == ["out"] and not general, (rows, counts, general)

    def after_unsorted(got):
        assert rows == [-1] and general == [True], (rows, general)
        assert K._rows_sorted_memo(ei) is False

    def after_sorted(got):
        assert rows == ["out"] and counts == ["out"] and not general, (rows, counts, general)

    steps = [
        Step("hub-cold", before=lambda: _assert(K._HUB_LISTS.get(ei) is None, "cold"), after=after_retry),
        Step("hub-warm", before=lambda: _assert(K._HUB_LISTS.get(ei) is not None, "hub list remembered"),
             after=after_hub_warm),
        Step("unsorted", change=lambda: ei.copy_(ei_u),
             before=lambda: _assert(K._HUB_LISTS.get(ei) is None and K._rows_sorted_memo(ei) is None, "version moved"),
             after=after_unsorted),
        Step("unsorted-warm", after=lambda got: _assert(not rows and general == [True], (rows, general))),
        Step("sorted-in-place", change=lambda: ei.copy_(ei_s),
             before=lambda: _assert(K._rows_sorted_memo(ei) is None, "version moved"), after=after_sorted),
    ]
    run_sequence(steps, call, reference, f"coalesce_{op}_{'w' if weighted else 'u'}")


def test_coalesce_hub_memo_is_keyed_on_the_list_alone(dev, monkeypatch):
    """Item 2, second half: ``_HUB_LISTS`` is keyed on the edge list, the hub row is a property of (list, clustering).
    The same ``edge_index`` with a clustering that makes no hub row is then run on the huge-row kernels (a cost, not a
    result), and the float64 form -- no huge-row kernels, reads no hub memo -- answers on the marked object as ever."""
    from tgp import kernels as K
    ei_h, _, _, cl_hub, cl_flat, w, k = WS.hub_data(7)
    ei, cl_hub, cl_flat, w = ei_h.to(dev), cl_hub.to(dev), cl_flat.to(dev), w.to(dev)
    idx_hub, idx_flat = K.build_assign_index(cl_hub, k), K.build_assign_index(cl_flat, k)
    counts = []
    _spy(monkeypatch, K, "_count_fill", counts, note=lambda r: r if isinstance(r, int) else "out")

    def check(cl, index, weights, case):
        pe, pw = K.coalesce_edges(ei, weights, cl, k, "sum", True, assign_index=index)
        if weights.dtype == torch.float64:
            rei, rw = WS._dense_ref_coalesce(ei.cpu(), weights.cpu(), cl.cpu(), k, "sum", True)
            assert torch.equal(pe.cpu(), rei)
            err = float(torch.linalg.vector_norm(pw.cpu() - rw) / torch.linalg.vector_norm(rw))
            print(f"FUZZ forward | {case} | edge_weight(f64) | e_kernel {err:.2e} | e_r32 nan | ratio nan")
            assert pw.dtype == torch.float64 and err <= F64_BOUND, err
            return
        r64, r32 = _coalesce_ref(ei, weights, cl, k, "sum")
        rep = []
        fails = WS.forward_errors(case, {"edge_index": pe, "edge_weight": pw}, r64, r32, exact=("edge_index",), report=rep)
        WS.print_report(rep)
        assert not fails, "\n".join(fails)

    check(cl_flat, idx_flat, w, "coalesce_flat-0:cold")
    assert K._HUB_LISTS.get(ei) is None and -5 not in counts
    check(cl_hub, idx_hub, w, "coalesce_hub-1:cold")
    assert K._HUB_LISTS.get(ei) is not None and -5 in counts
    del counts[:]
    check(cl_flat, idx_flat, w, "coalesce_flat-2:marked")  # the huge-row kernels on a list without a hub row
    assert -5 not in counts
    del counts[:]
    check(cl_hub, idx_hub, w.double(), "coalesce_hub-3:f64")  # float64: declines -5 for the hub row, the general route answers
    check(cl_flat, idx_flat, w.double(), "coalesce_flat-4:f64")
    assert K._HUB_LISTS.get(ei) is not None  # (float64 neither reads nor writes it)


# ==================================================================================================== 5. batch facts
SIZES_1 = [6, 0, 9, 5]    # n = 20, graph ids 0..3, id 1 without nodes
SIZES_2 = [4, 0, 3, 13]


def _batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def _check_info(info, batch):
    b = batch.cpu()
    sizes = torch.bincount(b)
    assert info.num_graphs == sizes.numel()
    assert torch.equal(info.sizes.cpu(), sizes)
    assert info.is_sorted == bool((b[1:] >= b[:-1]).all())
    assert info.max_nodes == int(sizes.max()) and info.distinct == int((sizes > 0).sum())
    assert torch.equal(info.ptr.cpu(), torch.cat([sizes.new_zeros(1), sizes.cumsum(0)]))
    assert info.sizes_host == sizes.tolist()


def _plan_of(sizes, ratio):
    """k_g as PyG computes it (float32 product, ceil), its prefix sums and total."""
    k = (float(ratio) * torch.tensor(sizes, dtype=torch.float32)).ceil().to(torch.long)
    return int(k.sum()), k, torch.cat([k.new_zeros(1), k.cumsum(0)])


def _check_plan(info, sizes, ratio):
    plan = info.memo.get(("topk", float(ratio)))
    assert plan is not None, (ratio, list(info.memo))
    total, k, koff = _plan_of(sizes, ratio)
    assert int(plan[0]) == total and torch.equal(plan[1].cpu(), k) and torch.equal(plan[2].cpu(), koff), (ratio, plan)
    if ("topk_total", float(ratio)) in info.memo:  # (there when the plan came with the facts launch)
        assert int(info.memo[("topk_total", float(ratio))]) == total


def _topk_selection_equals_oracle(batch, ratio, dev, seed=3):
    """TopkSelect on scores that cannot tie (a shuffled grid 3 / 19 apart, p = e_0: the dot product is exact) against
    the oracle's selection, exactly."""
    import tgp_oracle as O
    from tgp.select import TopkSelect
    g = torch.Generator().manual_seed(seed)
    n = batch.numel()
    x = torch.randn(n, 2, generator=g)
    x[:, 0] = torch.linspace(-1.5, 1.5, n)[torch.randperm(n, generator=g)]
    p = torch.tensor([[1.0, 0.0]])
    sel = TopkSelect(in_channels=2, ratio=ratio).to(dev)
    with torch.no_grad():
        sel.weight.copy_(p)
        so = sel(x.to(dev), batch=batch)
    ni, ci, w = O.topk_select(x, p, ratio, batch.cpu())
    assert torch.equal(so.node_index.cpu(), ni) and torch.equal(so.cluster_index.cpu(), ci)
    torch.testing.assert_close(so.weight.cpu(), w, rtol=1e-6, atol=1e-6)


def test_batch_facts_follow_in_place_changes(dev):
    """Item 5a: ``batch_info`` -> ``batch.copy_`` with other sizes -> the same vector made unsorted.  A repeated call is
    a memo hit (the same object), a changed vector a miss; every fact equals bincount / the sortedness check and
    TopkSelect equals the oracle's selection."""
    from tgp.utils import ops
    batch = _batch_of(SIZES_1).to(dev)
    info = ops.batch_info(batch)
    _check_info(info, batch)
    assert ops.batch_info(batch) is info and ops._INFO_OF_BATCH.get(batch) is info
    _topk_selection_equals_oracle(batch, 0.5, dev)
    batch.copy_(_batch_of(SIZES_2))
    assert ops._INFO_OF_BATCH.get(batch) is None
    info2 = ops.batch_info(batch)
    assert info2 is not info
    _check_info(info2, batch)
    _topk_selection_equals_oracle(batch, 0.5, dev)
    _check_plan(ops.batch_info(batch), SIZES_2, 0.5)
    batch.copy_(_batch_of(SIZES_2)[torch.randperm(20, generator=torch.Generator().manual_seed(1))])
    assert ops._INFO_OF_BATCH.get(batch) is None
    info3 = ops.batch_info(batch)
    assert not info3.is_sorted
    _check_info(info3, batch)
    _topk_selection_equals_oracle(batch, 0.5, dev)


def test_prefetched_batch_facts_are_dropped_after_an_in_place_change(dev):
    """Item 5b: prefetch -> in-place change -> ``batch_info``: the pending call describes the old contents and must not
    be read."""
    from tgp.utils import ops
    batch = _batch_of(SIZES_1).to(dev)
    ops.prefetch_batch_info(batch, 0.5)
    assert ops._PREFETCHED_FACTS.get(batch) is not None
    batch.copy_(_batch_of(SIZES_2))
    assert ops._PREFETCHED_FACTS.get(batch) is None
    info = ops.batch_info(batch, 0.5)
    _check_info(info, batch)
    _check_plan(info, SIZES_2, 0.5)
    _topk_selection_equals_oracle(batch, 0.5, dev)


@pytest.mark.parametrize("r1,r2", [(0.5, 0.3), (0.3, 0.5), (0.0, 0.5), (0.5, 0.0)])
def test_prefetched_topk_plan_belongs_to_its_ratio(dev, r1, r2):
    """Item 5c/d: a prefetch at ratio r1, read by ``batch_info`` at r2.  Whatever is stored under ("topk", r) must be the
    plan of r.  Regression: with both ratios > 0 and different, the prefetch's plan of r1 was stored under the key of r2
    (``ratio == ... or ratio > 0`` accepted it), and a TopkSelect at r2 would have kept r1's node counts."""
    from tgp.utils import ops
    batch = _batch_of(SIZES_1).to(dev)
    ops.prefetch_batch_info(batch, r1)
    pend = ops._PREFETCHED_FACTS.get(batch)
    assert pend is not None and pend[0] == float(r1)
    info = ops.batch_info(batch, r2)
    assert ops._PREFETCHED_FACTS.get(batch) is None
    _check_info(info, batch)
    for key in info.memo:
        if key[0] == "topk":
            _check_plan(info, SIZES_1, key[1])
    if r2 > 0:
        _check_plan(info, SIZES_1, r2)   # asked with a ratio: its plan came with the facts
        _topk_selection_equals_oracle(batch, r2, dev)
    else:
        _check_plan(info, SIZES_1, r1)   # the prefetch's plan is kept, under its own ratio
        _topk_selection_equals_oracle(batch, r1, dev)


def test_prefetched_batch_facts_whose_slot_was_reused_are_launched_again(dev):
    """Item 5e: prefetched calls rotate through eight pinned slots.  (a) One prefetch, then eight other facts launches
    on the stream: the slot was reused, ``batch_info`` must not wait for words that are gone and launches again.
    (b) Nine prefetches on nine vectors: ``_PREFETCHED_FACTS`` keeps eight, the first is forgotten and launched again;
    reading it takes the second one's slot, and so on down the line -- every vector still gets its own facts."""
    from tgp import _native as N
    from tgp import kernels as K
    from tgp.utils import ops
    state = K._sps_state(dev, N.stream_ptr(dev), 0)
    first = _batch_of(SIZES_1).to(dev)
    ops.prefetch_batch_info(first, 0.5)
    _, (held, tag, _, _, _) = ops._PREFETCHED_FACTS.get(first)
    assert held is state
    ei = torch.tensor([[0, 1, 2, 3], [1, 0, 3, 2]], device=dev)
    eb = torch.tensor([0, 0, 1, 1], device=dev)
    for _ in range(8):
        handle = K.edge_facts_launch(ei, eb)
        assert handle[0].wait_facts(handle[1])[1] == 0
    assert state.facts_tag - tag >= 8 and ops._PREFETCHED_FACTS.get(first) is not None
    before = state.facts_tag
    info = ops.batch_info(first, 0.5)
    assert state.facts_tag == before + 1  # launched again
    _check_info(info, first)
    _check_plan(info, SIZES_1, 0.5)
    _topk_selection_equals_oracle(first, 0.5, dev)

    vectors = []
    for i in range(9):
        sizes = [i + 1, 0, 12 - i, 7]
        vectors.append((_batch_of(sizes).to(dev), sizes))
    for b, _ in vectors:
        ops.prefetch_batch_info(b, 0.5)
    assert ops._PREFETCHED_FACTS.get(vectors[0][0]) is None and ops._PREFETCHED_FACTS.get(vectors[1][0]) is not None
    for b, sizes in vectors:
        info = ops.batch_info(b, 0.5)
        _check_info(info, b)
        _check_plan(info, sizes, 0.5)
    _topk_selection_equals_oracle(vectors[0][0], 0.5, dev)
    _topk_selection_equals_oracle(vectors[8][0], 0.5, dev)


# =============================================================================================== 8. - 10. per-stream state
def _consumers(dev, seed=211):
    """Every consumer of ``open_call()`` / ``next_epoch()`` on small inputs, each with its oracle: name -> thunk that
    runs it and asserts the result."""
    import tgp_oracle as O
    from tgp import kernels as K
    from tgp.select import GraclusSelect
    x, ei_a, _, ew, batch, _ = (t.to(dev) for t in WS.sps_data(seed))
    n = x.size(0)
    pooler = _make_pooler("topk", x.size(1), dev)
    g = torch.Generator().manual_seed(seed)
    kept = torch.sort(torch.randperm(n, generator=g)[: n // 2])[0]
    cl = (torch.arange(n) // 3)
    k = int(cl.max()) + 1
    sw = WS.symmetric_distinct_weights(ei_a.cpu(), n, seed)
    mask = (torch.rand(n, generator=g) < 0.4).to(torch.uint8)
    cl_d, kept_d, sw_d, mask_d = cl.to(dev), kept.to(dev), sw.to(dev), mask.to(dev)
    index = K.build_assign_index(cl_d, k)

    def within(case, got, r64, r32, exact):
        fails = WS.forward_errors(case, got, r64, r32, exact=exact)
        assert not fails, "\n".join(fails)

    def sps():
        got = _pooled(pooler, x, ei_a, ew, batch)
        assert not K.sparse_pool_small_declined(ei_a)
        so = got["_so"]
        fields = (so.node_index.cpu(), so.cluster_index.cpu(), so.weight.detach().cpu(), int(so.num_supernodes))
        r64, r32 = WS.pool_given_selection("topk", x.cpu(), ei_a.cpu(), ew.cpu(), batch.cpu(), fields)
        within("wrap:sps", {n_: got[n_] for n_ in r64}, r64, r32, ("batch", "edge_index"))

    def subgraph():
        pe, pw = K.filter_edges(ei_a, ew, kept_d, n, True)

        def run(dtype):
            rei, rw = O.sparse_connect(ei_a.cpu(), ew.cpu().to(dtype), kept, torch.arange(kept.numel()), n, kept.numel(), True)
            return {"edge_index": rei, "edge_weight": rw}
        r64, r32 = WS.both(run)
        within("wrap:subgraph", {"edge_index": pe, "edge_weight": pw}, r64, r32, ("edge_index",))

    def coalesce():
        pe, pw = K.coalesce_edges(ei_a, ew, cl_d, k, "sum", True, assign_index=index, route="staged")
        r64, r32 = _coalesce_ref(ei_a, ew, cl_d, k, "sum")
        within("wrap:coalesce", {"edge_index": pe, "edge_weight": pw}, r64, r32, ("edge_index",))

    def graclus():
        so = GraclusSelect()(ei_a, sw_d, num_nodes=n, batch=batch)
        assert torch.equal(so.cluster_index.cpu(), WS.greedy_clusters(ei_a.cpu(), sw, n))

    def mask_index():
        index_, _ = K.mask_index(mask_d)
        assert torch.equal(index_[0].cpu(), mask.nonzero().view(-1))

    def read_count():
        c = torch.tensor([12345], dtype=torch.int64, device=dev)
        assert K._read_count(c) == 12345

    return {"sps": sps, "subgraph": subgraph, "coalesce": coalesce, "graclus": graclus, "mask_index": mask_index,
            "read_count": read_count}


def test_epoch_wrap(dev, monkeypatch):
    """Item 8: the state of the current stream is set to ``_EPOCH_LIMIT - 4``; eight calls alternating over
    the consumers of ``open_call()`` / ``next_epoch()`` cross it (``next_epoch`` synchronises, zeroes the status words
    and restarts at 1), each equal to its oracle; afterwards the epoch is a small number and every consumer still
    answers.  Nothing here can wait without end: a device-side look-back spin is bounded at 2^20 looks per window
    (csrc/lookback.h, ``sps_lookback_finish``: ``if (++spins > (1 << 20))`` -> the tile refuses and the host takes the
    staged route), and the host's poll of the pinned word at 4 000 000 looks (``_SpsState._spin``), after which it
    synchronises and raises."""
    from tgp import _native as N
    from tgp import kernels as K
    runs = _consumers(dev)
    for run in runs.values():  # (warm: allocations, status-word counts, memos)
        run()
    state = K._sps_state(dev, N.stream_ptr(dev), 0)
    epochs = []
    real = K._SpsState.next_epoch

    def next_epoch(self):
        e = real(self)
        if self is state:
            epochs.append(e)
        return e

    monkeypatch.setattr(K._SpsState, "next_epoch", next_epoch)
    limit = K._EPOCH_LIMIT
    state.epoch = limit - 4
    for name in ["sps", "subgraph", "coalesce", "graclus", "mask_index", "read_count", "sps", "subgraph"]:
        runs[name]()
    assert K._sps_state(dev, N.stream_ptr(dev), 0) is state
    # limit - 3, limit - 2, limit - 1 (the last epoch of the buffer), then the wrap branch: 1, 2, 3, ...
    assert len(epochs) >= 8 and epochs[:3] == [limit - 3, limit - 2, limit - 1], epochs
    assert epochs[3:] == list(range(1, len(epochs) - 2)), epochs
    assert state.epoch == len(epochs) - 3 and int(state.host[0]) >> 34 == state.epoch
    for run in runs.values():
        run()
    assert epochs[3:] == list(range(1, len(epochs) - 2)) and state.epoch < 64, epochs


def test_state_replaced_while_a_prefetch_is_pending(dev):
    """Item 9: a prefetched facts call holds the state object it was launched on; a call that needs more status words
    than that state's buffer makes ``_sps_state`` build a new one.  The prefetch is then read from the OLD state's
    pinned words (right facts), the new state starts at epoch 1 on a fresh buffer, and its first calls equal their
    oracles."""
    from tgp import _native as N
    from tgp import kernels as K
    from tgp.select import GraclusSelect
    from tgp.utils import ops
    runs = _consumers(dev, seed=212)
    st = N.stream_ptr(dev)
    key = (dev.index, st)
    old = K._sps_state(dev, st, 0)
    if old.status.numel() > (1 << 16):  # (an earlier test grew it: start from a state of the default size)
        del K._SPS_STATE[key]
        old = K._sps_state(dev, st, 0)
    batch = _batch_of(SIZES_1).to(dev)
    ops.prefetch_batch_info(batch, 0.5)
    _, (held, tag, _, _, _) = ops._PREFETCHED_FACTS.get(batch)
    assert held is old
    # the one-launch GraclusSelect needs 2 + B / 4 words: B graphs of two nodes joined by one edge
    L = N.lib()
    B = 4 * old.status.numel()
    need = int(L.tgp_graclus_match_graphs_fused_status_words(B))
    assert need > old.status.numel()
    n = 2 * B
    a = torch.arange(0, n, 2)
    ei = torch.stack([torch.arange(n), torch.stack([a + 1, a], 1).reshape(-1)]).to(dev)
    big_batch = (torch.arange(n) // 2).to(dev)
    so = GraclusSelect()(ei, None, num_nodes=n, batch=big_batch)
    new = K._SPS_STATE[key]
    assert new is not old and new.status.numel() >= need
    assert new.epoch == 1, new.epoch
    assert int(so.num_supernodes) == B and torch.equal(so.cluster_index, big_batch)
    info = ops.batch_info(batch, 0.5)   # read from the old state's pinned words
    assert old.facts_tag == tag + 1     # (the big batch vector's own facts, launched before the state was replaced ...
    assert new.facts_tag == 0           #  ... and no launch on the new one: the prefetched words were read)
    _check_info(info, batch)
    _check_plan(info, SIZES_1, 0.5)
    runs["sps"]()
    runs["subgraph"]()
    runs["coalesce"]()
    assert K._SPS_STATE[key] is new and 4 <= new.epoch < 32, new.epoch


def test_two_streams_interleaved(dev, monkeypatch):
    """Item 10: the sequence of item 1 (TopK on the default stream, Graclus on a side stream, each with tensors of its
    own), four rounds interleaved step by step with ``wait_stream`` ordering.  Each stream's results are exact, the two
    states are distinct objects, and a call on one stream leaves the other stream's epoch where it was."""
    from tgp import _native as N
    from tgp import kernels as K
    main = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(dev)
    hits = []  # (host code of the two sequences never overlaps: one list serves both)
    _spy(monkeypatch, K, "_edge_ptr_memo", hits)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        steps_b, call_b, ref_b, _ = _sps_sequence("graclus", dev, True, "streams_side", hits, seed=103)
        st_side = N.stream_ptr(dev)
    main.wait_stream(side)
    steps_a, call_a, ref_a, _ = _sps_sequence("topk", dev, True, "streams_main", hits, seed=102)
    st_main = N.stream_ptr(dev)
    assert st_main != st_side
    k_main, k_side = (dev.index, st_main), (dev.index, st_side)

    def epoch_of(key):
        return K._SPS_STATE[key].epoch if key in K._SPS_STATE else 0

    def on_main(i, step):
        def call():
            e_side = epoch_of(k_side)
            got = call_a()
            assert epoch_of(k_side) == e_side, "a call on the default stream advanced the side stream's epoch"
            return got
        run_sequence([step], call, ref_a, "streams_main", first=i)

    def on_side(i, step):
        side.wait_stream(main)
        with torch.cuda.stream(side):
            if step.change is not None:
                step.change()
            if step.before is not None:
                step.before()
            e_main, e_side = epoch_of(k_main), epoch_of(k_side)
            got = call_b()
            assert epoch_of(k_main) == e_main, "a call on the side stream advanced the default stream's epoch"
            assert epoch_of(k_side) > e_side
            if step.after is not None:
                step.after(got)
        main.wait_stream(side)
        # (compared on the default stream, which now waits for the side stream's work)
        run_sequence([Step(step.name)], lambda: got, ref_b, "streams_side", first=i)

    for i, (sa, sb) in enumerate(zip(steps_a[:4], steps_b[:4])):
        on_main(i, sa)
        on_side(i, sb)
    s_main, s_side = K._SPS_STATE[k_main], K._SPS_STATE[k_side]
    assert s_main is not s_side and s_main.status.data_ptr() != s_side.status.data_ptr()
    assert s_main.pinned.data_ptr() != s_side.pinned.data_ptr()
    torch.cuda.synchronize(dev)


# ======================================================================================= 3. CSR offsets and edge groups
def _sorted_list(n, e, seed):
    g = torch.Generator().manual_seed(seed)
    r, c = torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)
    order = torch.argsort(r * n + c, stable=True)
    return torch.stack([r[order], c[order]])


def _dense_of(ei, w, rows, cols, dtype):
    a = torch.zeros(rows, cols, dtype=dtype)
    a.index_put_((ei[0], ei[1]), torch.ones(ei.size(1), dtype=dtype) if w is None else w.to(dtype), accumulate=True)
    return a


def test_csr_offsets_sequence(dev):
    """Item 3a: ``csr_offsets`` (``_ROW_OFFSETS``) under ``spmm_csr``, n = 40, E = 160, K = 5 (seeds 31, 32): cold, warm
    (the very table again), contents replaced in place (a miss; the table of the NEW rows), then the same object asked
    with another ``num_rows`` (its own table: the key holds the row count).  T = A S bit-identical to ``spmm_sorted``,
    which builds its offsets on every call, and within bounds of the float64 product."""
    from tgp import kernels as K
    n, e, k = 40, 160, 5
    ei_a, ei_b = _sorted_list(n, e, 31), _sorted_list(n, e, 32)
    g = torch.Generator().manual_seed(33)
    w, s = torch.rand(e, generator=g) + 0.25, torch.randn(n, k, generator=g)
    ei, wd, sd = ei_a.to(dev), w.to(dev), s.to(dev)
    rows = {"n": n}
    tables = []

    def call():
        rp = K.csr_offsets(ei, rows["n"])
        tables.append(rp)
        return {"t": K.spmm_csr(rp, ei, wd, rows["n"], sd), "row_ptr": rp}

    def reference():
        eic = ei.clone()
        cold = {"t": K.spmm_sorted(eic, wd, rows["n"], sd)}
        host = ei.cpu()
        counts = torch.bincount(host[0], minlength=rows["n"])
        ptr = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32)
        r64, r32 = WS.both(lambda dt: {"t": _dense_of(host, w, rows["n"], n, dt) @ s.to(dt), "row_ptr": ptr})
        return {"cold": cold, "bitwise": ["t"], "r64": r64, "r32": r32, "exact": ["row_ptr"]}

    steps = [
        Step("cold", before=lambda: _assert(K._ROW_OFFSETS.get(ei, extra=n) is None, "cold")),
        Step("warm", before=lambda: _assert(K._ROW_OFFSETS.get(ei, extra=n) is tables[-1], "a hit is meant"),
             after=lambda got: _assert(tables[-1] is tables[-2], "the remembered table")),
        Step("replaced", change=lambda: ei.copy_(ei_b),
             before=lambda: _assert(K._ROW_OFFSETS.get(ei, extra=n) is None, "version moved"),
             after=lambda got: _assert(tables[-1] is not tables[-2], "a new table")),
        Step("more-rows", change=lambda: rows.update(n=n + 8),
             before=lambda: _assert(K._ROW_OFFSETS.get(ei, extra=n + 8) is None, "another row count"),
             after=lambda got: _assert(got["row_ptr"].numel() == n + 9, "the table of the asked row count")),
        Step("rows-back", change=lambda: rows.update(n=n),
             after=lambda got: _assert(got["row_ptr"].numel() == n + 1, "the table of the asked row count")),
    ]
    run_sequence(steps, call, reference, "csr_offsets")


def test_sag_edge_groups_sequence(dev):
    """Item 3b: SAGPooling's scorer (``_SAG_GROUPS``: by destination in the forward, by source in the backward), n = 40,
    E = 160, F = 6 (seeds 41, 42).  Forward and dX after every step against sag_restatement in float64; then the same
    object asked with another node count gets offsets of that length."""
    import sag_restatement as SR
    from tgp import functions as Fn
    from tgp import kernels as K
    from fuzz_compare import grad_path_errors, print_grad_report
    n, e, f = 40, 160, 6
    ei_a, ei_b = _sorted_list(n, e, 41), _sorted_list(n, e, 42)
    g = torch.Generator().manual_seed(43)
    x, w_rel, w_root, bias = (torch.randn(n, f, generator=g), torch.randn(f, generator=g) * 0.4,
                              torch.randn(f, generator=g) * 0.4, torch.randn(1, generator=g) * 0.1)
    ei = ei_a.to(dev)
    wr, wo, bd = w_rel.to(dev), w_root.to(dev), bias.to(dev)

    def kernel():
        xg = x.to(dev).requires_grad_(True)
        return {"score": Fn.sag_score(xg, ei, wr, wo, bd, False, True)}, {"x": xg}

    def oracle(dtype):
        xg = x.to(dtype).requires_grad_(True)
        t = SR.raw_score(xg, ei.cpu(), w_rel.to(dtype), w_root.to(dtype), bias.to(dtype))
        return {"score": torch.tanh(t)}, {"x": xg}

    def step(case, hit):
        memo = K._SAG_GROUPS.get(ei)
        assert (memo is not None and (n, True) in memo and (n, False) in memo) == hit, (case, memo)
        held = None if memo is None else (memo[(n, True)], memo[(n, False)])
        rep, frep = [], []
        got = kernel()[0]["score"]
        r64, r32 = WS.both(lambda dt: {"score": oracle(dt)[0]["score"].detach()})
        fails = WS.forward_errors(case, {"score": got}, r64, r32, report=frep)
        fails += grad_path_errors(case, kernel, oracle, ["x"], report=rep)
        WS.print_report(frep)
        print_grad_report(case, rep)
        assert not fails, "\n".join(fails)
        memo = K._SAG_GROUPS.get(ei)
        assert memo is not None and (n, True) in memo and (n, False) in memo
        if hit:  # the very groups again
            assert memo[(n, True)] is held[0] and memo[(n, False)] is held[1]
        for by_dst in (True, False):  # what is remembered describes the list as it is now
            counts = torch.bincount(ei.cpu()[1 if by_dst else 0], minlength=n)
            assert torch.equal(memo[(n, by_dst)].row_ptr.cpu().long(), torch.cat([counts.new_zeros(1), counts.cumsum(0)]))

    step("sag-0:cold", False)
    step("sag-1:warm", True)
    ei.copy_(ei_b)
    step("sag-2:replaced", False)
    grp = K.sag_edge_group(ei, n + 8, by_destination=False)  # rows ascend: offsets alone
    counts = torch.bincount(ei.cpu()[0], minlength=n + 8)
    assert grp.row_ptr.numel() == n + 9 and torch.equal(grp.row_ptr.cpu().long(),
                                                        torch.cat([counts.new_zeros(1), counts.cumsum(0)]))
    assert K._SAG_GROUPS.get(ei)[(n, False)].row_ptr.numel() == n + 1
    step("sag-3:after-other-count", True)


def test_lapool_variation_sequence(dev):
    """Item 3c: ``lapool_variation`` on an edge list (``lapool_edge_group``: ``_SORTED_ROWS`` + ``_ROW_OFFSETS``), n = 40,
    E = 160, F = 5 (seeds 51, 52): cold, warm, a list with other rows copied in, an UNSORTED list copied in (the
    by-source index is built instead of the offsets)."""
    from tgp import kernels as K
    n, e, f = 40, 160, 5
    ei_a, ei_b = _sorted_list(n, e, 51), _sorted_list(n, e, 52)
    g = torch.Generator().manual_seed(53)
    x, w = torch.randn(n, f, generator=g), torch.rand(e, generator=g) + 0.25
    ei_c = ei_b[:, torch.randperm(e, generator=g)]
    ei, xd, wd = ei_a.to(dev), x.to(dev), w.to(dev)

    def call():
        return {"v": K.lapool_variation(xd, edge_index=ei, edge_weight=wd)}

    def restate(dt):
        import lapool_restatement as LR
        return {"v": LR.variation(x.to(dt), edge_index=ei.cpu(), edge_weight=w.to(dt))}

    def reference():
        r64, r32 = WS.both(restate)
        return {"cold": {"v": K.lapool_variation(xd, edge_index=ei.clone(), edge_weight=wd)}, "bitwise": ["v"],
                "r64": r64, "r32": r32}

    steps = [
        Step("cold", after=lambda got: _assert(K._ROW_OFFSETS.get(ei, extra=n) is not None
                                               and K._rows_sorted_memo(ei) is True, "facts remembered")),
        Step("warm", before=lambda: _assert(K._ROW_OFFSETS.get(ei, extra=n) is not None, "a hit is meant")),
        Step("replaced", change=lambda: ei.copy_(ei_b),
             before=lambda: _assert(K._ROW_OFFSETS.get(ei, extra=n) is None and K._rows_sorted_memo(ei) is None,
                                    "version moved")),
        Step("unsorted", change=lambda: ei.copy_(ei_c),
             before=lambda: _assert(K._rows_sorted_memo(ei) is None, "version moved"),
             after=lambda got: _assert(K._rows_sorted_memo(ei) is False and K._ROW_OFFSETS.get(ei, extra=n) is None,
                                       "an unsorted list has no CSR offsets")),
    ]
    run_sequence(steps, call, reference, "lapool_variation")


def test_graclus_select_output_does_not_hand_over_a_stale_csr(dev):
    """Item 3d: GraclusSelect attaches the int32 CSR offsets of the list it walked to its SelectOutput
    (``SelectOutput._edge_csr``, a stamp of its own).  After ``edge_index.copy_(other)`` SparseConnect with the OLD
    SelectOutput must not use them: the result equals the oracle on the new list (n = 40, E = 160, seeds 61, 62)."""
    import tgp_oracle as O
    from tgp.connect import SparseConnect
    from tgp.select import GraclusSelect
    n, e = 40, 160
    ei_a, ei_b = WS.graphs_edge_list([n], [e // 2], 61), WS.graphs_edge_list([n], [e // 2], 62)
    m = e
    w = torch.rand(m, generator=torch.Generator().manual_seed(63)) + 0.25
    ei, wd = ei_a.to(dev), w.to(dev)
    so = GraclusSelect()(ei, wd, num_nodes=n)
    assert so.edge_csr_for(ei) is not None, "the staged matcher hands its CSR offsets over"
    conn = SparseConnect()

    def check(case, host):
        pe, pw = conn(ei, so, edge_weight=wd)
        k = int(so.num_supernodes)
        r64, r32 = WS.both(lambda dt: dict(zip(("edge_index", "edge_weight"), O.sparse_connect(
            host, w.to(dt), torch.arange(n), so.cluster_index.cpu(), n, k))))
        rep = []
        fails = WS.forward_errors(case, {"edge_index": pe, "edge_weight": pw}, r64, r32, exact=("edge_index",), report=rep)
        WS.print_report(rep)
        assert not fails, "\n".join(fails)

    check("graclus_csr-0:same-list", ei_a)
    ei.copy_(ei_b)
    assert so.edge_csr_for(ei) is None, "the CSR offsets of the old contents must not be handed over"
    check("graclus_csr-1:other-list", ei_b)


# ============================================================================================================ 4. symmetry
from test_gpu_grad_paths import DenseCase, _dev, _graph_names  # noqa: E402


class WarmDenseCase(DenseCase):
    """A DenseCase whose device tensors LIVE across calls (the memos key on them); the host copies the oracle reads are
    refreshed from them after every in-place change."""

    def hold(self):
        dev = _dev()
        self.d_ei, self.d_ew, self.d_batch = self.ei.to(dev), self.ew.to(dev), self.batch.to(dev)
        return self

    def refresh(self):
        self.ew = self.d_ew.cpu()

    between = None  # runs between the forward and the backward (the facts launches of the "not known" step)

    def kernel(self):
        from tgp.poolers import get_pooler
        dev = _dev()
        pooler = get_pooler(self.alias, in_channels=self.f, k=self.k).to(dev).train()
        lin = pooler.selector.mlp.lins[0]
        with torch.no_grad():
            lin.weight.copy_(self.ws[0])
            lin.bias.copy_(self.bs[0])
        xg = self.x.to(dev).requires_grad_(True)
        out = pooler(x=xg, adj=self.d_ei, edge_weight=self.d_ew, batch=self.d_batch)
        names = _graph_names(out.x.grad_fn, out.edge_index.grad_fn, *(v.grad_fn for v in out.loss.values()))
        assert any(self.node in nm for nm in names), (self.name, names)
        if self.between is not None:
            self.between()
        outs = {"x": out.x, "adj": out.edge_index, "s": out.so.s}
        for i, (nm, v) in enumerate(out.loss.items()):
            outs[f"loss{i + 1}:{nm}"] = v
        return outs, {"x": xg, "W0": lin.weight, "b0": lin.bias, "ew": self.d_ew}


def _symmetric_weights(ei, n, seed):
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    _, inv = torch.unique(lo * n + hi, return_inverse=True)
    return (torch.rand(int(inv.max()) + 1, generator=g) + 0.25)[inv]


def _warm_case(alias, route, seed):
    """The smallest shapes that reach the two nodes: fewer than 64 graphs keeps a batch away from the one-wave-per-graph
    kernels; density 0 sends it to ``_PoolLargeFn`` (densified), density 2 to ``_PoolUnbatchedFn`` (rows route)."""
    node = "_PoolLargeFn" if route == "large" else "_PoolUnbatchedFn"
    case = WarmDenseCase(f"warm-{route}-{alias}", alias, [23, 14, 30], 6, 5, seed=seed, weighted=True, deg=5.0,
                         density=0.0 if route == "large" else 2.0, node=node)
    case.ew = _symmetric_weights(case.ei, case.x.size(0), seed + 7)
    return case.hold()


def _grad_step(case, route, report_as, show=True):
    """One training step's checks: every upstream path alone (``grad_path_errors``); returns the failures and which
    backward route ran.  ``show``: print the measured ratios (not those of a planted fault)."""
    from fuzz_compare import grad_path_errors, print_grad_report
    from tgp import functions as Fn
    before = dict(Fn.POOL_LARGE_STATS)
    rep = []
    fails = grad_path_errors(report_as, case.kernel, case.oracle, case.leaves, report=rep)
    if show:
        print_grad_report(report_as, rep)
    ran = {r for r in ("symmetric", "general") if Fn.POOL_LARGE_STATS[r] > before[r]}
    return fails, ran


def _per_direction(case):
    """Another factor for every direction of a pair: A is no longer symmetric."""
    case.d_ew.mul_(torch.where(case.d_ei[0] < case.d_ei[1], 1.5, 0.75))
    case.refresh()


@pytest.mark.parametrize("route", ["large", "rows"])
@pytest.mark.parametrize("alias", ["mincut", "diff"])
def test_symmetry_verdict_follows_the_weights(alias, route, monkeypatch):
    """Item 4, the dense poolers' training step on live (edge_index, edge_weight) objects (3 graphs of 23, 14, 30 nodes,
    K = 6, F = 5).  Symmetric weights: the verdict becomes True and the backward drops V = A^T S; a second step is a memo
    hit; ``edge_weight.mul_`` with a factor per direction: the verdict of the old version must not be read -- the
    gradients are those of the asymmetric A (every path against float64) and the general backward runs; made symmetric
    again in place: the symmetric backward is back."""
    import tgp.poolers as P
    from tgp import kernels as K
    case = _warm_case(alias, route, 1200 + (0 if alias == "mincut" else 10) + (0 if route == "large" else 1))
    monkeypatch.setattr(P, "_ROWS_ROUTE_DENSITY", case.density)
    monkeypatch.setattr(P, "_FOLD_SPARSE_INPUTS", True)
    sym_w = case.d_ew.clone()
    memo = lambda: K._adj_symmetric_memo(case.d_ei, case.d_ew)  # noqa: E731
    assert memo() is None
    fails, ran = _grad_step(case, route, f"{case.name}-0:symmetric-cold")
    assert not fails, "\n".join(fails)
    assert memo() is True and "symmetric" in ran, (memo(), ran)
    fails, ran = _grad_step(case, route, f"{case.name}-1:symmetric-warm")
    assert not fails, "\n".join(fails)
    assert memo() is True and ran == {"symmetric"}, (memo(), ran)
    _per_direction(case)
    assert memo() is None, "the verdict outlived the version of the weights"
    fails, ran = _grad_step(case, route, f"{case.name}-2:per-direction")
    assert not fails, "\n".join(fails)
    assert memo() is False and ran == {"general"}, (memo(), ran)
    case.d_ew.copy_(sym_w)  # the mirror case: asymmetric first, made symmetric in place
    case.refresh()
    assert memo() is None
    fails, ran = _grad_step(case, route, f"{case.name}-3:symmetric-again")
    assert not fails, "\n".join(fails)
    assert memo() is True and "symmetric" in ran, (memo(), ran)


def test_symmetry_verdict_not_known_takes_the_general_backward(monkeypatch):
    """Item 4, "not known": nine facts launches between the forward (which asks) and the backward (which reads) reuse the
    verdict's pinned slot.  The backward must then take the general route -- on a symmetric A both are right, and the
    gradients say so -- and nothing is remembered."""
    import tgp.poolers as P
    from tgp import kernels as K
    case = _warm_case("mincut", "large", 1230)
    monkeypatch.setattr(P, "_ROWS_ROUTE_DENSITY", case.density)
    ei = torch.tensor([[0, 1, 2, 3], [1, 0, 3, 2]], device=_dev())
    eb = torch.tensor([0, 0, 1, 1], device=_dev())

    def between():
        for _ in range(9):
            handle = K.edge_facts_launch(ei, eb)
            assert handle[0].wait_facts(handle[1])[1] == 0

    case.between = between
    fails, ran = _grad_step(case, "large", "warm-unknown-0:not-known")
    assert not fails, "\n".join(fails)
    assert ran == {"general"} and K._adj_symmetric_memo(case.d_ei, case.d_ew) is None, ran
    case.between = None
    fails, ran = _grad_step(case, "large", "warm-unknown-1:known")
    assert not fails, "\n".join(fails)
    assert "symmetric" in ran and K._adj_symmetric_memo(case.d_ei, case.d_ew) is True


@pytest.mark.parametrize("route", ["large", "rows"])
def test_a_stale_symmetry_verdict_is_caught_by_the_gradient_check(route, monkeypatch):
    """Item C: with ``_adj_symmetric_memo`` patched to answer True whatever the version, the step on the per-direction
    weights runs the symmetric backward on an asymmetric A (arithmetic on the same buffers: U in place of V).  The
    gradient check of item 4 must REPORT it: failures on the paths whose backward forms V."""
    import tgp.poolers as P
    from tgp import kernels as K
    case = _warm_case("mincut", route, 1240)
    monkeypatch.setattr(P, "_ROWS_ROUTE_DENSITY", case.density)
    _per_direction(case)
    monkeypatch.setattr(K, "_adj_symmetric_memo", lambda *a, **k: True)
    fails, ran = _grad_step(case, route, f"{case.name}-stale", show=False)
    assert ran == {"symmetric"}, ran
    flagged = {m.split("path ")[1].split(",")[0] for m in fails if "path " in m}
    assert "adj" in flagged and any(p.startswith("loss1") for p in flagged), (flagged, fails)
    assert "x" not in flagged, flagged  # X' = S^T X never reads A


class HeldDenseCase:
    """A [B, N, N] adjacency the caller holds (``AdjSymmetry.of_dense``), B = 2, N = 20, K = 6, F = 5."""

    def __init__(self, alias, seed):
        from test_gpu_grad_paths import _linears
        g = torch.Generator().manual_seed(seed)
        self.alias, self.name = alias, f"warm-held-{alias}"
        a = torch.rand(2, 20, 20, generator=g) * (torch.rand(2, 20, 20, generator=g) < 0.3)
        a = torch.triu(a, 1)
        self.adj = a + a.transpose(1, 2)
        self.x = torch.randn(2, 20, 5, generator=g)
        self.ws, self.bs = _linears([5, 6], seed + 1)
        self.leaves = ["x", "W0", "b0"]
        self.d_adj = self.adj.to(_dev())

    def refresh(self):
        self.adj = self.d_adj.cpu()

    def oracle(self, dtype):
        import tgp_oracle as O
        lv = {"x": self.x.to(dtype).requires_grad_(True), "W0": self.ws[0].to(dtype).requires_grad_(True),
              "b0": self.bs[0].to(dtype).requires_grad_(True)}
        ref = O.dense_pool(self.alias, lv["x"], self.adj.to(dtype), None, None, [lv["W0"]], [lv["b0"]])
        outs = {"x": ref["x"], "adj": ref["edge_index"], "s": ref["s"]}
        for i, (n, v) in enumerate(ref["loss"].items()):
            outs[f"loss{i + 1}:{n}"] = v
        return outs, lv

    def kernel(self):
        from tgp.poolers import get_pooler
        dev = _dev()
        pooler = get_pooler(self.alias, in_channels=5, k=6).to(dev).train()
        lin = pooler.selector.mlp.lins[0]
        with torch.no_grad():
            lin.weight.copy_(self.ws[0])
            lin.bias.copy_(self.bs[0])
        xg = self.x.to(dev).requires_grad_(True)
        out = pooler(x=xg, adj=self.d_adj)
        names = _graph_names(out.x.grad_fn, out.edge_index.grad_fn, *(v.grad_fn for v in out.loss.values()))
        assert any("_PoolLargeFn" in nm for nm in names), names
        outs = {"x": out.x, "adj": out.edge_index, "s": out.so.s}
        for i, (n, v) in enumerate(out.loss.items()):
            outs[f"loss{i + 1}:{n}"] = v
        return outs, {"x": xg, "W0": lin.weight, "b0": lin.bias}


@pytest.mark.parametrize("alias", ["mincut", "diff"])
def test_symmetry_of_a_held_dense_adjacency(alias):
    """Item 4, ``of_dense``: a symmetric [B, N, N] adjacency, two steps, then ``adj[0, 3, 5] += 1``: the verdict of the
    old version must not be read, the gradients are those of the changed adjacency; ``adj[0, 5, 3] += 1`` restores the
    symmetry in place."""
    from tgp import kernels as K
    case = HeldDenseCase(alias, 1250 if alias == "mincut" else 1260)
    memo = lambda: K._adj_symmetric_memo(case.d_adj, None)  # noqa: E731
    for i, (change, verdict, route) in enumerate([(None, True, "symmetric"), (None, True, "symmetric"),
                                                  ((0, 3, 5), False, "general"), ((0, 5, 3), True, "symmetric")]):
        if change is not None:
            case.d_adj[change] += 1
            case.refresh()
            assert memo() is None, "the verdict outlived the version of the adjacency"
        elif i == 1:
            assert memo() is True
        fails, ran = _grad_step(case, "large", f"{case.name}-{i}:{route}")
        assert not fails, "\n".join(fails)
        assert memo() is verdict and route in ran and (i == 0 or ran == {route}), (i, memo(), ran)


def test_coalesced_memo_follows_in_place_changes(dev):
    """Item 4, ``_STRICTLY_SORTED`` (``coalesced_memo``; ``functions.coalesce_sum`` reads and writes it): a coalesced
    list is remembered as such; duplicates copied in: not remembered, and the duplicates are summed; coalesced again in
    place: remembered again.  Values against the float64 dense sum."""
    from tgp import functions as Fn
    from tgp import kernels as K
    n = 24
    key = torch.unique(torch.randint(0, n * n, (120,), generator=torch.Generator().manual_seed(71)))
    clean = torch.stack([key // n, key % n])
    dup = WS.with_duplicates(clean)
    w = torch.rand(clean.size(1), generator=torch.Generator().manual_seed(72)) + 0.25
    ei, wd = clean.to(dev), w.to(dev)

    def check(case, host, coalesced):
        pe, pw = Fn.coalesce_sum(ei, wd, n)
        assert K.coalesced_memo(ei, n) == coalesced, (case, K.coalesced_memo(ei, n))
        assert (pe is ei) == coalesced
        dense = lambda dt: _dense_of(host, w, n, n, dt)  # noqa: E731
        got = torch.zeros(n, n, dtype=torch.float64).index_put_((pe.cpu()[0], pe.cpu()[1]), pw.cpu().double(), accumulate=True)
        assert torch.equal(pe.cpu(), dense(torch.float64).nonzero().t())  # row-major, every pair once
        fails = WS.forward_errors(case, {"a": got}, {"a": dense(torch.float64)}, {"a": dense(torch.float32)})
        assert not fails, "\n".join(fails)

    check("coalesced-0:clean", clean, True)
    check("coalesced-1:warm", clean, True)
    ei.copy_(dup)
    assert not K.coalesced_memo(ei, n), "the fact outlived the version"
    check("coalesced-2:duplicates", dup, False)
    ei.copy_(clean)
    assert not K.coalesced_memo(ei, n)
    check("coalesced-3:clean-again", clean, True)


def test_hosc_loss_symmetry_and_coalescedness_follow_the_list(dev):
    """Item 4, losses: HOSC's loss terms on an un-padded, unweighted list of one graph (N = 24, K = 4, seed 75) read two
    facts of the ``edge_index`` object: "coalesced" (``_STRICTLY_SORTED``: the list is used as it is) and "symmetric"
    (``of_edge_list``: the backward skips A^T (A^T (A^T S))).  Symmetric list -> warm -> a directed list of the same E
    copied in (gradients of the asymmetric A) -> duplicates copied in (summed: entries of weight 2) -> the symmetric
    list again.  (DMoN's losses in utils/losses.py ask for neither fact: their backward forms no transposed product.)"""
    import hosc_restatement as HR
    from fuzz_compare import grad_path_errors, print_grad_report
    from tgp import kernels as K
    from tgp.utils import losses as L
    n, kc, alpha = 24, 4, 0.5
    sym = WS.graphs_edge_list([n], [40], 75)
    g = torch.Generator().manual_seed(76)
    key = torch.unique(torch.randint(0, n * n, (400,), generator=g))
    key = key[key // n != key % n]
    key = key[torch.randperm(key.numel(), generator=g)[: sym.size(1)]].sort()[0]
    directed = torch.stack([key // n, key % n])
    assert directed.shape == sym.shape
    dup = WS.with_duplicates(sym)
    logits = torch.randn(n, kc, generator=g)
    ei = sym.to(dev)
    state = {"host": sym}

    def kernel():
        lg = logits.to(dev).requires_grad_(True)
        terms = L.hosc_sparse_loss_terms(ei, None, torch.softmax(lg, -1), None, alpha=alpha, mu=0.0)
        return {"hosc": terms[0]}, {"logits": lg}

    def oracle(dtype):
        lg = logits.to(dtype).requires_grad_(True)
        s = torch.softmax(lg, -1).unsqueeze(0)
        a = _dense_of(state["host"], None, n, n, dtype).unsqueeze(0)
        return {"hosc": ((1 - alpha) * HR.cut_terms(a, s) + alpha * HR.ho_cut_terms(a, s)) / kc}, {"logits": lg}

    def step(case, host, coalesced, verdict):
        if host is not state["host"]:
            ei.copy_(host)
            state["host"] = host
            assert K._adj_symmetric_memo(ei, None) is None and not K.coalesced_memo(ei, n), (case, "version moved")
        rep, frep = [], []
        r64, r32 = WS.both(lambda dt: {"hosc": oracle(dt)[0]["hosc"].detach()})
        fails = WS.forward_errors(case, {"hosc": kernel()[0]["hosc"].detach()}, r64, r32, report=frep)
        fails += grad_path_errors(case, kernel, oracle, ["logits"], report=rep)
        WS.print_report(frep)
        print_grad_report(case, rep)
        assert not fails, "\n".join(fails)
        assert K.coalesced_memo(ei, n) == coalesced, case
        assert K._adj_symmetric_memo(ei, None) is verdict, (case, K._adj_symmetric_memo(ei, None))

    step("hosc_loss-0:symmetric", sym, True, True)
    step("hosc_loss-1:warm", sym, True, True)
    step("hosc_loss-2:directed", directed, True, False)
    step("hosc_loss-3:duplicates", dup, False, None)  # (the coalesced copy is a tensor of the call: nothing to remember)
    step("hosc_loss-4:symmetric-again", sym, True, True)


# ===================================================================================================== 6. NDP preparation
def test_ndp_inputs_follow_in_place_changes(dev):
    """Item 6: ``_NDP_INPUTS`` remembers the CSR offsets and the symmetrised (max) weights of a clean list per
    (edge_index, edge_weight, n).  n = 30, seed 81.  Weights changed in place so that the symmetrised maximum changes;
    the same ``edge_index`` without weights, then with them again: the remembered weights are those of the call's own
    inputs and the partition equals that of fresh clones (same generator seed) exactly."""
    from tgp.select import NDPSelect, _NDP_INPUTS
    n = 30
    g = torch.Generator().manual_seed(81)
    key = torch.unique(torch.randint(0, n * n, (90,), generator=g))
    r, c = key // n, key % n
    r, c = r[r != c], c[r != c]
    key = torch.unique(torch.cat([r * n + c, c * n + r]))
    host = torch.stack([key // n, key % n])
    w = torch.rand(host.size(1), generator=g) + 0.25   # one weight per DIRECTION: the symmetrised weight is their max
    ei, wd = host.to(dev), w.to(dev)
    sel = NDPSelect()

    def select(e, ww):
        torch.manual_seed(5)  # (a graph whose sign cut is below 0.5 gets the reference's random partition)
        so = sel(e, ww, num_nodes=n)
        return so.node_index.clone(), int(so.num_supernodes)

    def sym_max(ww):
        d = torch.zeros(n, n)
        d[host[0], host[1]] = ww
        return torch.maximum(d, d.t())[host[0], host[1]]

    def step(case, ww_dev, ww_host, hit):
        assert (_NDP_INPUTS.get(ei, ww_dev, n) is not None) == hit, (case, "hit expected" if hit else "miss expected")
        got = select(ei, ww_dev)
        prep = _NDP_INPUTS.get(ei, ww_dev, n)
        assert prep is not None, case
        if ww_host is not None:  # what is remembered belongs to THESE weights
            assert torch.equal(prep[1].cpu(), sym_max(ww_host)), case
        with WS.cold_memos():
            want = select(ei.clone(), None if ww_dev is None else ww_dev.clone())
        assert got[1] == want[1] and torch.equal(got[0], want[0]), (case, got, want)

    step("ndp-0:cold", wd, w, False)
    step("ndp-1:warm", wd, w, True)
    factor = torch.where(host[0] < host[1], 3.0, 0.2)
    wd.mul_(factor.to(dev))
    assert not torch.equal(sym_max(w * factor), sym_max(w))
    step("ndp-2:weights-changed", wd, w * factor, False)
    step("ndp-3:no-weights", None, None, False)
    step("ndp-4:weights-again", wd, w * factor, False)
    step("ndp-5:warm", wd, w * factor, True)


# ===================================================================================================== 7. shared products
def test_shared_products_are_not_reused_after_an_in_place_change(dev):
    """Item 7: DenseConnect's and the link loss' forwards share U = A S and V = A^T S through ``functions.shared_products``
    (stamps of S and adj).  Two such pairs in one step on the same ``adj``, changed in place in between: the second pair
    must form its own products.  B = 2, N = 24, K = 65 (K > 64: U is a tensor of its own), seed 91; values and the
    gradients of the second pair against float64."""
    from fuzz_compare import grad_path_errors, print_grad_report
    from tgp import functions as Fn
    from tgp.connect import _DenseConnectFn
    from tgp.utils.losses import _LinkNormFn
    g = torch.Generator().manual_seed(91)
    B, n, k = 2, 24, 65
    logits = torch.randn(B, n, k, generator=g)
    adj = torch.rand(B, n, n, generator=g) * (torch.rand(B, n, n, generator=g) < 0.3)
    d_adj = adj.to(dev)
    state = {"adj": adj}

    def kernel():
        lg = logits.to(dev).requires_grad_(True)
        s = torch.softmax(lg, -1)
        raw = _DenseConnectFn.apply(s, d_adj)
        link = _LinkNormFn.apply(s, d_adj)
        kernel.products = Fn.shared_products(s, d_adj)
        kernel.s = s
        return {"raw": raw, "link": link}, {"logits": lg}

    def oracle(dtype):
        lg = logits.to(dtype).requires_grad_(True)
        s, a = torch.softmax(lg, -1), state["adj"].to(dtype)
        return {"raw": s.transpose(1, 2) @ a @ s, "link": torch.linalg.matrix_norm(a - s @ s.transpose(1, 2)).square().sum().sqrt()}, {"logits": lg}

    def check(case):
        rep, frep = [], []
        outs, _ = kernel()
        r64, r32 = WS.both(lambda dt: {n_: v.detach() for n_, v in oracle(dt)[0].items()})
        fails = WS.forward_errors(case, {n_: v.detach() for n_, v in outs.items()}, r64, r32, report=frep)
        fails += grad_path_errors(case, kernel, oracle, ["logits"], report=rep)
        WS.print_report(frep)
        print_grad_report(case, rep)
        assert not fails, "\n".join(fails)

    # one step, two pairs: the first pair's products are formed (its backward runs) before adj changes
    outs, lv = kernel()
    first, s1 = kernel.products, kernel.s
    assert Fn.shared_products(s1, d_adj) is first, "both forwards of a pair share one object"
    torch.autograd.grad([outs["raw"].sum(), outs["link"]], [lv["logits"]])
    assert first.u is not None and first.v is not None
    check("shared_products-0:first")
    d_adj[0, 3, 5] += 1
    state["adj"] = d_adj.cpu()
    assert not first.matches(s1, d_adj) and Fn.shared_products(s1, d_adj) is not first
    check("shared_products-1:adj-changed")
