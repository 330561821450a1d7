#!/usr/bin/env python3
"""Generate the golden vectors of EigenPooling (``tests/golden/golden_eigenpool_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_lapool.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs ``EigenPooling`` as
it is (scikit-learn 1.7.2 and scipy are installed there) on small seeded inputs: symmetric graphs with planted blocks
and generic random edge weights in [0.1, 1).

The reference's labels come from scikit-learn's k-means; with ``numpy.random.seed`` set they repeat, and they are
stored.  ``kind = "sklearn"`` cases keep them, ``kind = "planted"`` cases replace ``_cluster_from_adj`` by the planted
partition (that is how group sizes 1, 2, below H and above 16, and an empty cluster in the middle of a graph, get in).
Every case also stores a float64 run of the reference GIVEN THE SAME LABELS, the gradient of ``sum(x_pool ** 2)`` with
respect to ``x`` from it, and per (graph, cluster) ``err_ref = max |Theta_fp32 - Theta_f64|``.

A case is kept only if every cluster of two or more nodes passes
  (a) gaps of at least 1e-3 between consecutive eigenvalues among the first min(H + 1, m) of the float64 spectrum,
  (b) |v[0]| >= 1e-3 for every used mode, so rounding cannot flip the sign rule,
  (c) the float64 and the fp32 run of the reference agree on every sign (err_ref far below a flipped vector's 2 |v|).
Seeds are walked until a case passes; the seed is stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eigenpool.py
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as G  # noqa: E402,F401  (installs the PyG stand-in and imports the reference)
from tgp.poolers.eigenpool import EigenPooling  # noqa: E402

RS = sys.modules["tgp.select.eigenpool_select"]  # (``tgp.select.eigenpool_select`` itself names the function)
import eigenpool_restatement as R  # noqa: E402

OPTS = [dict(remove_self_loops=True, degree_norm=True, edge_weight_norm=False, sparse_output=False),
        dict(remove_self_loops=False, degree_norm=False, edge_weight_norm=True, sparse_output=False),
        dict(remove_self_loops=True, degree_norm=True, edge_weight_norm=True, sparse_output=True)]
_ORIG_CLUSTER = RS._cluster_from_adj


def planted_graphs(blocks_per_graph, seed, p_in=0.8, p_out=0.04, self_loops=False):
    """Symmetric block graphs: (edge_index, edge_weight, batch, planted labels)."""
    g = torch.Generator().manual_seed(seed)
    eis, ews, bs, labs, off = [], [], [], [], 0
    for gi, blocks in enumerate(blocks_per_graph):
        lab = torch.cat([torch.full((s,), c, dtype=torch.long) for c, s in enumerate(blocks)])
        n = lab.numel()
        same = lab.view(-1, 1) == lab.view(1, -1)
        prob = torch.where(same, torch.tensor(p_in), torch.tensor(p_out))
        up = torch.triu(torch.rand(n, n, generator=g) < prob, 1)
        w = torch.triu(torch.rand(n, n, generator=g) * 0.9 + 0.1, 1) * up
        a = w + w.t()
        if self_loops:
            a = a + torch.diag(torch.rand(n, generator=g) * 0.9 + 0.1)
        idx = a.nonzero().t()
        eis.append(idx + off)
        ews.append(a[idx[0], idx[1]])
        bs.append(torch.full((n,), gi, dtype=torch.long))
        labs.append(lab)
        off += n
    return torch.cat(eis, 1), torch.cat(ews), torch.cat(bs), torch.cat(labs)


def run(cfg, opts, x, ei, ew, batch, labels_per_graph=None, record=None):
    """One forward + lift of the reference; labels_per_graph replaces the clustering, record collects its labels."""
    queue = None if labels_per_graph is None else list(labels_per_graph)

    def cluster(adj_np, k):
        if queue is not None:
            lab = queue.pop(0).numpy().astype(np.int64)
            return lab, max(1, min(k, adj_np.shape[0]))
        lab, actual = _ORIG_CLUSTER(adj_np, k)
        if record is not None:
            record.append(torch.as_tensor(lab, dtype=torch.long))
        return lab, actual

    RS._cluster_from_adj = cluster
    try:
        pooler = EigenPooling(k=cfg["k"], num_modes=cfg["num_modes"], normalized=cfg["normalized"], **opts).eval()
        xr = x.clone().requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = pooler(x=xr, adj=ei, edge_weight=ew, batch=batch)
        if queue is not None:
            queue = list(labels_per_graph)
        lift = pooler(x=out.x.detach(), so=out.so, batch=batch, lifting=True)
    finally:
        RS._cluster_from_adj = _ORIG_CLUSTER
    return xr, out, lift


def same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def adj_record(out):
    if out.edge_weight is None:
        return {"dense": out.edge_index.detach().clone()}
    return {"edge_index": out.edge_index.clone(), "edge_weight": out.edge_weight.detach().clone()}


def make_case(name, kind, blocks_per_graph, cfg, feat, seed0, single=False, self_loops=False, need_planted=False):
    for seed in range(seed0, seed0 + 200):
        ei, ew, batch, planted = planted_graphs(blocks_per_graph, seed, self_loops=self_loops)
        n = planted.numel()
        x = torch.randn(n, feat, generator=torch.Generator().manual_seed(seed + 7))
        b = None if single else batch
        slices = R.graph_slices(b, n)
        if kind == "sklearn":
            np.random.seed(seed)
            rec = []
            run(cfg, OPTS[0], x, ei, ew, b, record=rec)
            per_graph = rec  # one entry per graph: _cluster_from_adj's own rules (k >= n, k = 1) included
            assert len(per_graph) == len(slices)
        else:
            per_graph = [planted[lo:hi] for lo, hi in slices]
        labels = torch.cat(per_graph)
        width = cfg["k"] if not single else max(1, min(cfg["k"], n))
        matches = all(same_partition(labels[lo:hi], planted[lo:hi]) for lo, hi in slices)
        if need_planted and not matches:
            continue
        # fp32 and float64 runs of the reference on these labels
        x32, out32, lift32 = run(cfg, OPTS[0], x, ei, ew, b, labels_per_graph=per_graph)
        x64, out64, lift64 = run(cfg, OPTS[0], x.double(), ei, ew.double(), b, labels_per_graph=per_graph)
        th32 = out32.so.theta if isinstance(out32.so.theta, list) else [out32.so.theta]
        th64 = out64.so.theta if isinstance(out64.so.theta, list) else [out64.so.theta]
        ok, err_ref = True, torch.zeros(len(slices) * width, dtype=torch.float64)
        H = cfg["num_modes"]
        for gi, (lo, hi) in enumerate(slices):
            a = R.dense_adjacency(ei, ew.double(), lo, hi)
            for c in range(width):
                nodes = (labels[lo:hi] == c).nonzero().view(-1)
                m = nodes.numel()
                if m == 0:
                    continue
                cols = [h * width + c for h in range(H)]
                err_ref[gi * width + c] = (th32[gi][nodes][:, cols].double() - th64[gi][nodes][:, cols]).abs().max()
                if m == 1:
                    continue
                modes, lam = R.cluster_modes(a[nodes][:, nodes], H, cfg["normalized"], R.TINY[torch.float64])
                used = min(H + 1, m)
                if (lam[1:used] - lam[:used - 1]).min() < 1e-3 or modes[0].abs().min() < 1e-3:
                    ok = False
                if err_ref[gi * width + c] > 0.05:
                    ok = False
        if not ok:
            continue
        (g64,) = torch.autograd.grad((out64.x ** 2).sum(), x64)
        exp32 = {"theta": [t.clone() for t in th32], "x_pool": out32.x.detach().clone(), "lift": lift32.detach().clone(),
                 "adj": []}
        exp64 = {"theta": [t.clone() for t in th64], "x_pool": out64.x.detach().clone(), "lift": lift64.detach().clone(),
                 "adj": [], "grad_x": g64.clone()}
        for opts in OPTS:
            # (the reference's sparse edge_weight_norm needs a pooled batch vector: one graph gets a batch of zeros there)
            bo = torch.zeros(n, dtype=torch.long) if b is None and opts["sparse_output"] else b
            exp32["adj"].append(adj_record(run(cfg, opts, x, ei, ew, bo, labels_per_graph=per_graph)[1]))
            exp64["adj"].append(adj_record(run(cfg, opts, x.double(), ei, ew.double(), bo, labels_per_graph=per_graph)[1]))
        sizes = torch.bincount((torch.zeros(n, dtype=torch.long) if b is None else b) * width + labels,
                               minlength=len(slices) * width)
        return {"kind": kind, "seed": seed, "cfg": dict(cfg), "width": width,
                "inputs": {"x": x, "edge_index": ei, "edge_weight": ew, "batch": b},
                "labels": labels, "planted": planted, "ref_matches_planted": bool(matches),
                "group_sizes": sizes, "expected": exp32, "f64": exp64, "err_ref": err_ref}
    raise RuntimeError(f"no seed passed for {name}")


def main():
    cases = {}
    base = dict(k=4, num_modes=3, normalized=True)
    # the probe of the issue: six graphs, one below k (every node its own cluster)
    cases["eig_batch6"] = make_case("eig_batch6", "sklearn", [[3], [2, 3, 2, 2], [4, 3, 4, 3], [5, 5, 5, 5], [9, 8, 8, 8],
                                                                [3, 4, 3, 4]], base, 5, 100)
    # planted partitions that scikit-learn recovers (the labeller test compares against these)
    cases["eig_single20"] = make_case("eig_single20", "sklearn", [[7, 6, 7]], dict(k=3, num_modes=5, normalized=True), 4,
                                      200, single=True, need_planted=True)
    cases["eig_batch3"] = make_case("eig_batch3", "sklearn", [[5, 5, 4], [7, 7, 6], [11, 11, 11]],
                                    dict(k=3, num_modes=4, normalized=True), 6, 300, need_planted=True)
    cases["eig_single33"] = make_case("eig_single33", "sklearn", [[9, 8, 8, 8]], dict(k=4, num_modes=3, normalized=True), 5,
                                      400, single=True, need_planted=True)
    # planted labels: group sizes 1, 2, below H, above 16, an empty cluster in the middle of a graph, self-loops
    planted = [[1, 2, 3, 3], [20, 0, 4, 3], [2, 5, 7, 0]]
    cases["eig_planted"] = make_case("eig_planted", "planted", planted, dict(k=4, num_modes=5, normalized=True), 5, 500,
                                     self_loops=True)
    cases["eig_planted_unnormalized"] = make_case("eig_planted_unnormalized", "planted", planted,
                                                  dict(k=4, num_modes=5, normalized=False), 5, 600, self_loops=True)
    # k >= n on one graph: one cluster per node, every mode the node's self-loop weight
    cases["eig_k_above_n"] = make_case("eig_k_above_n", "sklearn", [[5, 4]], dict(k=12, num_modes=3, normalized=True), 3,
                                       700, single=True, self_loops=True)
    sizes = torch.cat([c["group_sizes"] for c in cases.values()])
    H_max = 5
    assert (sizes == 1).any() and (sizes == 2).any() and ((sizes > 2) & (sizes < H_max)).any() and (sizes > 16).any()
    assert sum(c["ref_matches_planted"] and c["kind"] == "sklearn" and c["cfg"]["k"] < c["labels"].numel()
               for c in cases.values()) >= 3
    path = os.path.join(HERE, "golden_eigenpool_v1.pt")
    torch.save({"tgp_version": "1.0.1", "opts": OPTS, "cases": cases}, path)
    for name, c in cases.items():
        print(name, "seed", c["seed"], "groups", c["group_sizes"].tolist(), "err_ref max", float(c["err_ref"].max()),
              "matches planted", c["ref_matches_planted"])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
