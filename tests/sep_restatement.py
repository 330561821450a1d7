"""The one-level SEP selector (Wu et al., ICML 2022; reference select/sep_select.py) stated once: float64, brute-force
argmin over a table of every live pair, no heap.  DESIGN 4.26 is the prose form.

Per graph: self-loops dropped, ``A`` symmetric (every listed edge lands at ``[i][j]`` and ``[j][i]``, duplicates add up
in edge-list order), a zero entry is "not adjacent".  Per connected component (ordered by smallest node): leaves, greedy
merging by the minimum of ``(delta, a, b)`` over adjacent live pairs (ids are creation ids), compression to height 2 by
the minimum of ``(child_cut * ln(vol_parent / vol_u), u)``, then labels: the root's internal children in creation order,
then its leaf children as singletons in ascending node order.

``arith="f64"`` keeps the cut table in float64.  ``arith="kernel"`` is the device kernel's arithmetic: the table is
float32 (entries added in edge-list order, a merged row is the float32 sum of its two rows), row sums add the float32
entries in ascending column order into float64, everything else is float64.

``gaps`` (a dict) collects ``min_ratio``: over every decision, the smallest ``|value - best| / scale`` of a candidate
whose inputs differ from the best one's, ``scale`` being the largest absolute term of the two candidates' sums.  Two
candidates are a tie only if their input tuples are equal as unordered pairs; equal values from different inputs are a
ratio of 0.  The input tuple of a merge is what its three terms are computed from: ``(v - g, v_ab / v)`` per side (an
unordered pair) and ``(cut, v_ab)``; a side with ``v - g == 0`` -- every leaf -- contributes an exact zero in any IEEE
arithmetic whatever its quotient is, so there the quotient is left out.  Equal tuples give equal bits wherever the same
expression is evaluated, which is what lets the id tie-break decide them identically on the host and on the device.  A
compression's tuple is ``(child_cut, vol_parent / vol_u)``.  A fixture or a seed is usable for an exact-label check only
if that ratio is well above rounding.
"""
import math

import numpy as np

_LN2 = math.log(2.0)
_ln = np.frompyfunc(math.log, 1, 1)  # math.log itself, elementwise: log2(x) = ln(x) / ln(2) as math.log(x, 2) computes it


def _log(x):
    return _ln(np.asarray(x, dtype=np.float64)).astype(np.float64)


def _delta(va, ga, vb, gb, cut, VOL):
    """(delta, scale) of merging a and b; arrays or scalars, float64."""
    vab = va + vb
    t1 = (va - ga) * (_log(vab / va) / _LN2)
    t2 = (vb - gb) * (_log(vab / vb) / _LN2)
    t3 = 2 * cut * (_log(VOL / vab) / _LN2)
    d = (t1 + t2 - t3) / VOL
    scale = np.maximum(np.maximum(np.abs(t1), np.abs(t2)), np.abs(t3)) / VOL
    return d, scale


def _note(gaps, ratio):
    if gaps is not None:
        gaps["min_ratio"] = min(gaps.get("min_ratio", math.inf), float(ratio))


def dense_adjacency(n, src, dst, w, arith="f64"):
    """The symmetric table of one graph (local indices); ValueError for a non-finite or negative summed weight."""
    dt = np.float32 if arith == "kernel" else np.float64
    A = np.zeros((n, n), dtype=dt)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    w = np.ones(src.shape[0], dtype=dt) if w is None else np.asarray(w).astype(dt)
    keep = src != dst
    i, j, w = src[keep], dst[keep], w[keep]
    rows, cols = np.stack([i, j], 1).ravel(), np.stack([j, i], 1).ravel()
    np.add.at(A, (rows, cols), np.repeat(w, 2))  # unbuffered: in edge-list order
    if not np.isfinite(A).all() or (A < 0).any():
        raise ValueError("sep: edge weights must be finite and non-negative after duplicates are summed")
    return A


def components(A):
    """Lists of nodes (ascending), ordered by smallest node."""
    n = A.shape[0]
    seen, out = np.zeros(n, dtype=bool), []
    for s in range(n):
        if seen[s]:
            continue
        seen[s] = True
        stack, comp = [s], []
        while stack:
            u = stack.pop()
            comp.append(u)
            for v in np.nonzero(A[u])[0].tolist():
                if not seen[v]:
                    seen[v] = True
                    stack.append(v)
        out.append(sorted(comp))
    return out


def component_clusters(sub, gaps=None):
    """Clusters (lists of positions in ``sub``, label order) of one connected component with at least two nodes."""
    m = sub.shape[0]
    M = 2 * m - 1
    C = np.zeros((M, M), dtype=sub.dtype)
    C[:m, :m] = sub
    vol = np.zeros(M)
    vol[:m] = np.cumsum(sub.astype(np.float64), axis=1)[:, -1]  # ascending column order, float64
    VOL = float(np.cumsum(vol[:m])[-1])
    g, cc = vol.copy(), np.zeros(M)
    parent, height = np.full(M, -1), np.zeros(M, dtype=np.int64)
    live = np.zeros(M, dtype=bool)
    live[:m] = True
    D, S = np.full((M, M), np.inf), np.zeros((M, M))
    a, b = np.nonzero(np.triu(sub != 0, 1))
    D[a, b], S[a, b] = _delta(vol[a], g[a], vol[b], g[b], sub[a, b].astype(np.float64), VOL)

    def key(x, y):
        # what the candidate's three terms are computed from: (v - g, v_ab / v) per side and (cut, v_ab).  A side with
        # v - g == 0 (every leaf) contributes an exact zero whatever its quotient is, so its quotient is no input
        vab = vol[x] + vol[y]
        p, q = [(vol[z] - g[z], vab / vol[z] if vol[z] - g[z] != 0 else 0.0) for z in (x, y)]
        return (min(p, q), max(p, q), float(C[x, y]), vab)

    # ---- merging
    for t in range(m, M):
        flat = int(np.argmin(D))  # the first minimum in row-major order: the minimum of (delta, a, b), a < b
        a, b = divmod(flat, M)
        assert np.isfinite(D[a, b]), "a connected component always has an adjacent live pair"
        if gaps is not None:
            xs, ys = np.nonzero(np.isfinite(D))
            scale = np.maximum(S[xs, ys], S[a, b])
            gap = D[xs, ys] - D[a, b]
            ratio = np.where(scale > 0, gap / np.where(scale > 0, scale, 1.0), 0.0)
            best = key(a, b)
            for i in np.nonzero(ratio < 1e-3)[0].tolist():
                if (xs[i], ys[i]) != (a, b) and key(int(xs[i]), int(ys[i])) != best:
                    _note(gaps, ratio[i])
        cut = float(C[a, b])
        C[t, :] = C[a, :] + C[b, :]
        C[:, t] = C[t, :]
        C[t, t] = 0
        for dead in (a, b):
            D[dead, :], D[:, dead], live[dead], parent[dead] = np.inf, np.inf, False, t
        live[t] = True
        vol[t], g[t], cc[t] = vol[a] + vol[b], g[a] + g[b] - 2 * cut, cut
        height[t] = max(height[a], height[b]) + 1
        xs = np.nonzero(live & (C[t, :] != 0))[0]
        xs = xs[xs != t]
        if xs.size:
            D[xs, t], S[xs, t] = _delta(vol[xs], g[xs], vol[t], g[t], C[xs, t].astype(np.float64), VOL)
    root = M - 1

    # ---- compressing to height 2
    alive = np.ones(M, dtype=bool)
    while True:
        h, depth = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
        for u in range(M):  # a parent's id is larger than its children's
            if alive[u] and u != root:
                h[parent[u]] = max(h[parent[u]], h[u] + 1)
        if h[root] <= 2:
            break
        for u in range(M - 2, -1, -1):
            if alive[u]:
                depth[u] = depth[parent[u]] + 1
        cand = [(cc[u] * math.log(vol[parent[u]] / vol[u]), u) for u in range(m, M - 1)
                if alive[u] and depth[u] + h[u] > 2]
        val, u = min(cand)
        if gaps is not None:
            best = (cc[u], vol[parent[u]] / vol[u])  # the product's two factors: child_cut and the quotient
            for v, w in cand:
                if w != u and (cc[w], vol[parent[w]] / vol[w]) != best:
                    scale = max(abs(v), abs(val))
                    _note(gaps, (v - val) / scale if scale > 0 else 0.0)
        p = parent[u]
        parent[(parent == u) & alive] = p
        cc[p] += cc[u]
        alive[u] = False

    # ---- labels
    clusters = [[x for x in range(m) if parent[x] == u] for u in range(m, M - 1) if alive[u] and parent[u] == root]
    clusters += [[x] for x in range(m) if parent[x] == root]
    return clusters


def graph_labels(n, src, dst, w=None, arith="f64", gaps=None):
    """(labels [n] as a list, number of clusters) of one graph given by local indices."""
    if n == 0:
        return [], 0
    A = dense_adjacency(n, src, dst, w, arith)
    labels, k = [-1] * n, 0
    if not A.any():
        return list(range(n)), n
    for comp in components(A):
        if len(comp) == 1:
            groups = [[0]]
        else:
            groups = component_clusters(A[np.ix_(comp, comp)], gaps)
        for grp in groups:
            for x in grp:
                labels[comp[x]] = k
            k += 1
    return labels, k


def sep_select(num_nodes, edge_index, edge_weight=None, batch=None, arith="f64", gaps=None):
    """(cluster_index [N] int64 array, num_supernodes) of a batch: per-graph labels offset by the exclusive prefix of the
    per-graph counts, in graph order.  ValueError for an edge between two graphs."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    w = None if edge_weight is None else np.asarray(edge_weight).reshape(-1)
    bt = np.zeros(num_nodes, dtype=np.int64) if batch is None else np.asarray(batch, dtype=np.int64)
    if ei.size and (ei.min() < 0 or ei.max() >= num_nodes):
        raise ValueError("sep: an edge endpoint out of range")
    if ei.size and (bt[ei[0]] != bt[ei[1]]).any():
        raise ValueError("sep: an edge whose endpoints lie in two graphs")
    out, off = np.full(num_nodes, -1, dtype=np.int64), 0
    local = np.zeros(num_nodes, dtype=np.int64)
    for gidx in range(int(bt.max()) + 1 if num_nodes else 0):
        nodes = np.nonzero(bt == gidx)[0]
        if nodes.size == 0:
            continue
        local[nodes] = np.arange(nodes.size)
        e = np.nonzero(bt[ei[0]] == gidx)[0] if ei.size else np.zeros(0, dtype=np.int64)
        lab, k = graph_labels(nodes.size, local[ei[0, e]], local[ei[1, e]], None if w is None else w[e], arith, gaps)
        out[nodes] = np.asarray(lab, dtype=np.int64) + off
        off += k
    return out, off
