"""Helpers of tests/test_gpu_warm_state.py: the driver that takes an operator through cold call -> warm call -> in-place
change -> call again on the SAME tensor objects, the float64 restatements the results are held against, and the host
data of the sequences.  No tests here.

The library remembers facts per tensor object + version (``tgp._memo.TensorMemo``) and per (device, stream)
(``tgp.kernels._SpsState``); which kernel a call launches, and which device tables it is handed, depends on what is
remembered.  A sweep that builds fresh tensors for every call only ever sees the cold side of that.  Here a step
changes the live tensors with ordinary in-place torch operations (``copy_``, ``mul_``, ``index_put_``; never through
``.data`` -- the documented blind spot of ``tgp.clear_memos``) and never changes a shape, the node count or the edge
count: every remembered offset table, permutation or range a wrong implementation might hand to a kernel still indexes
inside the buffers of the new contents, so a stale fact shows as a wrong VALUE, not as an access out of bounds.
"""
import contextlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from fuzz_compare import CAP, FACTOR, conditioning, forward_errors, print_report  # noqa: E402


# ----------------------------------------------------------------------------------------------------------- the driver
@contextlib.contextmanager
def cold_memos():
    """Inside the block the package remembers nothing (``tgp.clear_memos()``), whatever runs there starts cold; on the
    way out the facts of the live tensors are put back, so the sequence outside goes on warm.  (The entries go back
    into the memos' own dicts: the weak-reference callbacks of ``TensorMemo.put`` close over them.)"""
    import tgp
    from tgp import _memo
    saved = [(m, dict(m._d)) for m in _memo._ALL]
    tgp.clear_memos()
    try:
        yield
    finally:
        for m, d in saved:
            m._d.clear()
            m._d.update(d)


class Step:
    """One step of a sequence.  ``change()`` alters the live tensors in place (None: call again as they are);
    ``before()`` asserts the memo state the change must have left (a miss after the version moved, a hit where the
    call is meant to be warm); ``after(outputs)`` asserts the state the call must leave behind."""

    def __init__(self, name, change=None, before=None, after=None):
        self.name, self.change, self.before, self.after = name, change, before, after


def run_sequence(steps, call, reference, case="sequence", report=None, factor=FACTOR, first=0):
    """After every step: ``call()`` on the live objects (-> outputs by name) against ``reference()``, which is evaluated
    on clones taken at that moment with every memo cleared (:func:`cold_memos`) and returns a dict with

      cold     outputs of the library's cold call on the clones (by the same names),
      bitwise  names that must equal ``cold`` bit for bit (integer outputs, floats documented as identical between routes),
      r64,r32  the float64 CPU restatement and its float32 twin,
      exact    names of ``r64`` compared with ``torch.equal`` (integer outputs).

    Float outputs go through ``fuzz_compare.forward_errors`` with the project's FACTOR / FLOOR / CAP; a draw whose float32
    restatement alone exceeds CAP / FACTOR fails here as ill-conditioned (change the seed, never the cap).
    ``first``: the number of the first step (a sequence driven one step at a time).  Returns the outputs of every step."""
    seen = []
    for i, step in enumerate(steps, first):
        where = f"{case}-{i}:{step.name}"
        if step.change is not None:
            step.change()
        if step.before is not None:
            step.before()
        got = call()
        if step.after is not None:
            step.after(got)
        with cold_memos():
            ref = reference()
        fails = []
        for name in ref.get("bitwise", ()):
            a, b = got[name], ref["cold"][name]
            if (a is None) != (b is None) or (a is not None and not (a.shape == b.shape and torch.equal(a, b))):
                fails.append(f"{where}: output {name} differs from the cold call on clones")
        r64, r32 = ref["r64"], ref["r32"]
        cond = conditioning(r64, r32)
        if cond > CAP / FACTOR:
            fails.append(f"{where}: conditioning {cond:.3e} above CAP / FACTOR = {CAP / FACTOR:.3e}: redraw the data")
        rep = []
        live = {k: v for k, v in got.items() if v is not None and k in r64}
        fails += forward_errors(where, live, r64, r32, exact=tuple(ref.get("exact", ())), factor=factor, report=rep)
        print_report(rep)
        if report is not None:
            report.extend(rep)
        assert not fails, "\n".join(fails)
        seen.append(got)
    return seen


def both(fn):
    """``fn(dtype)`` in float64 and float32 -> (r64, r32)."""
    return fn(torch.float64), fn(torch.float32)


# ------------------------------------------------------------------------------------------------ float64 restatements
def _dense_ref_coalesce(ei, w, cl, k, op, remove_self_loops, eps=1e-8):
    """Differentiable torch restatement of cluster -> coalesce(reduce=op) -> filters, returning the pooled weights in
    row-major order (what PyG's scatter-based coalesce + postprocess_adj_pool_sparse compute)."""
    key = cl[ei[0]] * k + cl[ei[1]]
    uniq, inv = torch.unique(key, return_inverse=True)
    if op in ("sum", "mean"):
        out = torch.zeros(uniq.numel(), dtype=w.dtype).index_add(0, inv, w)
        if op == "mean":
            out = out / torch.bincount(inv, minlength=uniq.numel()).to(w.dtype)
    elif op == "mul":
        out = torch.ones(uniq.numel(), dtype=w.dtype).scatter_reduce(0, inv, w, "prod", include_self=True)
    else:
        out = torch.zeros(uniq.numel(), dtype=w.dtype).scatter_reduce(0, inv, w, "amax" if op == "max" else "amin",
                                                                     include_self=False)
    r, c = uniq // k, uniq % k
    keep = out.abs() > eps
    if remove_self_loops:
        keep = keep & (r != c)
    return torch.stack([r[keep], c[keep]]), out[keep]


def pool_given_selection(alias, x, ei, ew, batch, so_fields, reduce_op="sum"):
    """(r64, r32) of the oracle's sparse Reduce + Connect on host tensors, given the selection the product made
    (``so_fields``: node_index, cluster_index, weight or None, num_supernodes -- host tensors).  Select's own agreement
    with the oracle is the business of the selector tests; Reduce and Connect are what the one-launch kernel computes."""
    import tgp_oracle as O
    ni, ci, w, k = so_fields

    def run(dtype):
        xx = x.to(dtype)
        ww = None if ew is None else ew.to(dtype)
        if alias == "topk":
            sw = w.to(dtype)
            xp = O.reduce_sparse(xx, ni, ci, sw, k)
            bp = O.reduce_batch_sparse(batch, ni, ci, k)
            rei, rew = O.sparse_connect(ei, ww, ni, ci, x.size(0), k, True, "sum", False, bp, False)
        else:
            ref = O.cluster_pool(xx, ei, ww, batch, ci, k, reduce_op=reduce_op)
            xp, bp, rei, rew = ref["x"], ref["batch"], ref["edge_index"], ref["edge_weight"]
        out = {"x": xp.to(dtype), "batch": bp, "edge_index": rei}
        if rew is not None:
            out["edge_weight"] = rew
        return out

    return both(run)


# --------------------------------------------------------------------------------------------------- data of the sequences
SPS_SIZES = [3, 17, 64, 40, 9]            # 5 sorted graphs of 3 to 64 nodes, one of exactly 64
SPS_PAIRS_A = [2, 20, 90, 50, 8]          # undirected pairs per graph of list A ...
SPS_PAIRS_B = [3, 30, 70, 60, 7]          # ... and of list B: the same E = 340, other per-graph edge counts


def graphs_edge_list(sizes, pairs, seed):
    """Row-major sorted, duplicate-free undirected edge list with ``pairs[g]`` pairs inside graph g."""
    g = torch.Generator().manual_seed(seed)
    keys, off, n = [], 0, sum(sizes)
    for size, m in zip(sizes, pairs):
        iu = torch.triu_indices(size, size, 1)
        assert m <= iu.size(1)
        pick = iu[:, torch.randperm(iu.size(1), generator=g)[:m]] + off
        keys += [pick[0] * n + pick[1], pick[1] * n + pick[0]]
        off += size
    key = torch.sort(torch.cat(keys))[0]
    return torch.stack([key // n, key % n])


def sps_data(seed, f=5):
    """x [133, F], two edge lists of E = 340, weights (a few below eps), the sorted batch vector and a second batch
    vector whose boundary between graphs 1 and 2 moved by one node, so that an edge of list A and of list B joins two
    graphs (sizes 3, 18, 63, 40, 9: still no graph beyond 64 nodes)."""
    g = torch.Generator().manual_seed(seed)
    n = sum(SPS_SIZES)
    ei_a = graphs_edge_list(SPS_SIZES, SPS_PAIRS_A, seed + 1)
    ei_b = graphs_edge_list(SPS_SIZES, SPS_PAIRS_B, seed + 2)
    assert ei_a.shape == ei_b.shape
    batch = torch.repeat_interleave(torch.arange(len(SPS_SIZES)), torch.tensor(SPS_SIZES))
    moved = batch.clone()
    first = SPS_SIZES[0] + SPS_SIZES[1]    # first node of graph 2 joins graph 1
    moved[first] = 1
    for ei in (ei_a, ei_b):                # that node has an edge into graph 2 in both lists
        if not bool((ei[0] == first).any()):
            raise AssertionError("redraw: the moved node has no edge")
    x = torch.randn(n, f, generator=g)
    ew = torch.rand(ei_a.size(1), generator=g) + 0.25
    ew[torch.rand(ei_a.size(1), generator=g) < 0.05] = 0.0
    return x, ei_a, ei_b, ew, batch, moved


def hub_data(seed, n=200, k=30, hub_nodes=120, hub_entries=1100, other=400):
    """Row-sorted list of E = 1500 entries on n = 200 nodes whose supernode row 0 (``cl_hub``: the first 120 nodes) holds
    more than 1024 raw entries; ``cl_flat`` spreads the same nodes over all k supernodes (no row beyond ~100 entries);
    ``ei_unsorted``: a list of the same E without a hub under ``cl_hub`` (rows among the other nodes), rows in random
    order, and ``ei_resorted`` the same entries row-sorted."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.cat([torch.randint(0, hub_nodes, (hub_entries,), generator=g),
                      torch.randint(hub_nodes, n, (other,), generator=g)])
    cols = torch.randint(0, n, (rows.numel(),), generator=g)
    order = torch.argsort(rows * n + cols, stable=True)
    ei = torch.stack([rows[order], cols[order]])
    cl_hub = torch.cat([torch.zeros(hub_nodes, dtype=torch.long),
                        1 + torch.arange(n - hub_nodes) % (k - 1)])
    cl_flat = torch.arange(n) % k
    e = ei.size(1)
    r2 = torch.randint(hub_nodes, n, (e,), generator=g)   # rows outside the hub cluster: <= ~60 entries per supernode row
    c2 = torch.randint(0, n, (e,), generator=g)
    ei_unsorted = torch.stack([r2, c2])
    assert not bool((r2[1:] >= r2[:-1]).all())
    ei_resorted = ei_unsorted[:, torch.argsort(r2 * n + c2, stable=True)]
    w = torch.rand(e, generator=g) + 0.5
    w[torch.rand(e, generator=g) < 0.03] = 0.0
    return ei, ei_unsorted, ei_resorted, cl_hub, cl_flat, w, k


def symmetric_distinct_weights(ei, n, seed):
    """One weight per undirected pair, all different: the heavy-edge matching of such a list is unique (the sequential
    greedy matching), whatever the order the rounds find it in."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    uniq, inv = torch.unique(lo * n + hi, return_inverse=True)
    w = torch.rand(uniq.numel(), generator=g) + 0.1
    assert torch.unique(w).numel() == w.numel()
    return w[inv]


def greedy_clusters(ei, w, n):
    """Consecutive cluster ids of the sequential greedy heavy-edge matching on distinct symmetric weights
    (label = min of the pair, then ``unique``'s inverse: select/graclus_select.py:66-70)."""
    lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    keep = lo < hi
    key, first = torch.unique(lo[keep] * n + hi[keep], return_inverse=True)
    pw = torch.zeros(key.numel(), dtype=w.dtype).scatter_(0, first, w[keep])
    label = torch.arange(n)
    free = [True] * n
    for j in torch.argsort(pw, descending=True).tolist():
        a, b = int(key[j]) // n, int(key[j]) % n
        if free[a] and free[b]:
            free[a] = free[b] = False
            label[a] = label[b] = min(a, b)
    return torch.unique(label, return_inverse=True)[1]


def with_duplicates(ei):
    """The same shape, every second entry a repeat of its predecessor: still row-major sorted, no longer coalesced."""
    dup = ei.clone()
    m = dup[:, 1::2].size(1)
    dup[:, 1::2] = ei[:, 0::2][:, :m]
    return dup
