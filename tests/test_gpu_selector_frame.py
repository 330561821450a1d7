"""The per-graph frame the k-MIS and the edge-contraction selector share (csrc/graph_frame.h): where it finds a graph's
edges, where its LDS cache ends, where the workgroup size steps, and what it refuses.

Every case is a sorted batch of three graphs, the interesting one between two small ones so that a wrong node or edge
range shows in its neighbours.  Inside a graph the sources ascend and the targets are random: duplicates and self-loops
occur.  Every case runs the natural call and the forced device-wide call and compares both, exactly, with the plain-torch
restatements (tests/kmis_restatement.py with order_k 1 and 2, tests/edgepool_restatement.py) under a random permutation.
No input is meant to fault anything: the refusals are the ones the kernels have.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import edgepool_restatement as RE  # noqa: E402
import kmis_restatement as RK  # noqa: E402

pytestmark = pytest.mark.gpu

# name: (nodes per graph, edge entries per graph, what is done to the list, max_graph_nodes declared (None: the longest))
CASES = {
    # the cache of a 64-node frame holds 16 * 64 = 1024 entries: one below, exactly, one beyond
    "cache64_1023": ([5, 64, 7], [8, 1023, 9], None, None),
    "cache64_1024": ([5, 64, 7], [8, 1024, 9], None, None),
    "cache64_1025": ([5, 64, 7], [8, 1025, 9], None, None),
    # the cache of a 256-node frame is the full 4096: one entry read from global memory
    "cache256_4097": ([9, 256, 3], [12, 4097, 4], None, None),
    # 64 / 256 / 1024 threads: the longest graph on either side of both steps
    "threads_64": ([5, 64, 7], [8, 300, 9], None, None),
    "threads_65": ([5, 65, 7], [8, 300, 9], None, None),
    "threads_256": ([9, 256, 3], [12, 700, 4], None, None),
    "threads_257": ([9, 257, 3], [12, 700, 4], None, None),
    "empty_graph": ([6, 0, 11], [9, 0, 14], None, None),
    # refused, then exact on the device-wide route
    "shuffled": ([5, 64, 7], [8, 300, 9], "shuffle", None),
    "crossing": ([5, 64, 7], [8, 300, 9], "cross", None),
    "longer_than_declared": ([10, 70, 10], [14, 150, 12], None, 40),  # the frame of 40 holds 64 nodes, the graph has 70
}
DECLINED = ("shuffled", "crossing", "longer_than_declared")


def build(name):
    """(edge_index, n, ptr, max_graph_nodes, generator) on the host."""
    sizes, entries, edit, declared = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.long)
    ptr[1:] = torch.tensor(sizes).cumsum(0)
    parts = []
    for i, (n_g, m) in enumerate(zip(sizes, entries)):
        if m == 0:
            continue
        src = torch.randint(0, n_g, (m,), generator=g).sort()[0]
        parts.append(torch.stack([src, torch.randint(0, n_g, (m,), generator=g)]) + ptr[i])
    ei = torch.cat(parts, 1)
    if edit == "shuffle":
        ei = ei[:, torch.randperm(ei.size(1), generator=g)]
        assert bool((ei[0, 1:] < ei[0, :-1]).any())
    elif edit == "cross":
        e = entries[0] + entries[1] // 2  # an entry of the middle graph now ends in the last one; the sources still ascend
        ei[1, e] = ptr[2] + 1
    return ei.contiguous(), int(ptr[-1]), ptr, declared if declared is not None else max(sizes), g


def kmis_reference(ei, n, k, perm):
    mis, cluster = RK.mis_cluster(ei, k, perm, n)
    return int(mis.sum()), mis.nonzero().view(-1), cluster


def check_kmis(res, ref, n, what):
    assert res.k == ref[0], what
    assert torch.equal(res.mis, ref[1]), what
    assert torch.equal(res.index[1], ref[2]), what
    assert torch.equal(res.index[0], torch.arange(n, device=res.index.device)), what


def edgepool_reference(ei, n, perm):
    match = RE.matching(ei, n, perm)
    cluster, k = RE.clusters(ei, n, match)
    return k, match, cluster


def check_edgepool(res, ref, n, what):
    assert res.k == ref[0], what
    assert torch.equal(res.matched.bool(), ref[1]), what
    assert torch.equal(res.match, ref[1].nonzero().view(-1)), what
    assert torch.equal(res.index[1], ref[2]), what
    assert torch.equal(res.index[0], torch.arange(n, device=res.index.device)), what


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("selector", ["kmis", "edgepool"])
def test_frame(selector, name):
    from tgp import _native, kernels
    dev = torch.device("cuda:0")
    ei, n, ptr, gmax, g = build(name)
    ei, ptr = ei.to(dev), ptr.to(dev)
    if selector == "kmis":
        perm = torch.randperm(n, generator=g).to(dev)
        runs = [(lambda k=k, **kw: kernels.kmis_select(ei, n, k, perm=perm, graph_ptr=ptr, max_graph_nodes=gmax, **kw),
                 check_kmis, kmis_reference(ei, n, k, perm)) for k in (1, 2)]
    else:
        perm = torch.randperm(ei.size(1), generator=g).to(dev)
        runs = [(lambda **kw: kernels.edge_contract_select(ei, n, graph_ptr=ptr, max_graph_nodes=gmax, perm=perm, **kw),
                 check_edgepool, edgepool_reference(ei, n, perm))]
    for call, check, ref in runs:  # (each reference is computed once and compared with both routes)
        natural = call()
        assert natural.route == ("rounds" if name in DECLINED else "graphs"), (selector, name, natural.route)
        check(natural, ref, n, (selector, name, "natural"))
        forced = call(route="rounds")
        assert forced.route == "rounds"
        check(forced, ref, n, (selector, name, "rounds"))
        if name in ("shuffled", "crossing"):
            with pytest.raises(_native.TgpNativeError, match="declined"):
                call(route="graphs")
