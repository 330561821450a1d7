"""Structural-entropy pooling (SEP: Wu et al., ICML 2022; reference poolers/sep.py, select/sep_select.py).

Select grows, per graph, a coding tree by greedy merging (the pair whose merge lowers the structural entropy most),
compresses it to height 2 and takes the root's children as clusters: a hard assignment of every node to one depth-1
cluster.  Reduce, Connect and Lift are ``BaseReduce``, ``SparseConnect`` and ``BaseLift``.  DESIGN 4.26 states the
algorithm; ``tests/sep_restatement.py`` is its brute-force float64 form.

Routes.  Device batches with float32 (or no) edge weights and a sorted batch vector take ``tgp_sep_select_f32``: one
workgroup per graph, all graphs in one launch, one host wait per call (the status word and the supernode count).  Graphs
of more than ``kernels.sep_max_nodes()`` nodes, float64 weights, host tensors and an unsorted batch vector take the same
algorithm on the host in float64 with a lazy heap; a batch may mix both routes and labels come back in graph order.
The selector accepts host tensors (the reference's selector is host code too); Reduce, Connect and Lift stay device-only.

Only the one-level selector is built: ``levels > 1`` needs the reference's ``leaf_up`` / ``root_down`` passes and raises
``NotImplementedError``.

**Deviations from the reference.**  Edge weights must be finite and non-negative after duplicates are summed, anything
else raises ``ValueError`` (the reference then fails inside ``math.log`` or not at all, depending on the graph).  An edge
whose endpoints lie in two graphs raises ``ValueError`` (the reference drops it).  The root's leaf children become
singleton clusters in ascending node order (the reference's order there is Python's ``set`` iteration order, which is
ascending in almost every case).  The symmetric table holds every listed edge at ``[i][j]`` and ``[j][i]``: a uniform
factor 2 against the reference's ``to_undirected`` on a list that names both directions, to which every decision is
invariant.
"""
from __future__ import annotations

import heapq
import math
from typing import List, Optional, Tuple, Union

import torch
from torch import Tensor

from .. import kernels as K
from ..connect import SparseConnect
from ..lift import BaseLift
from ..reduce import BaseReduce
from ..select import Select, SelectOutput
from ..src import BasePrecoarseningMixin, PoolingOutput, SRCPooling
from ..utils.ops import batch_info, connectivity_to_edge_index

_LEVELS_MESSAGE = ("SEP with levels > 1 needs the coding tree's leaf_up / root_down passes, which this build does not "
                   "have: only the one-level selector (levels=1) is built")
_BAD_WEIGHT = "sep_select: edge weights must be finite and non-negative after duplicates are summed"
_BAD_INDEX = ("sep_select: an index outside its table (an edge endpoint or edge position out of range, or an edge whose "
              "endpoints lie in two graphs); nothing out of range was read")


# ------------------------------------------------------------------------------------------------ host route
def _merge_delta(va: float, ga: float, vb: float, gb: float, cut: float, VOL: float) -> float:
    vab = va + vb
    return ((va - ga) * math.log(vab / va, 2) + (vb - gb) * math.log(vab / vb, 2)
            - 2 * cut * math.log(VOL / vab, 2)) / VOL


def _host_component(nodes: List[int], adj: List[dict]) -> List[List[int]]:
    """Clusters (lists of nodes, label order) of one connected component with at least two nodes."""
    m = len(nodes)
    rank = {u: i for i, u in enumerate(nodes)}
    nb = [{rank[v]: w for v, w in adj[u].items()} for u in nodes]  # live cluster -> {adjacent live cluster: cut}
    vol = [0.0] * m
    for i in range(m):
        s = 0.0
        for v in sorted(nb[i]):  # ascending column order
            s += nb[i][v]
        vol[i] = s
    VOL = 0.0
    for v in vol:
        VOL += v
    g, cc, parent, dead = list(vol), [0.0] * m, [-1] * m, [False] * m
    heap = [(_merge_delta(vol[a], g[a], vol[b], g[b], w, VOL), a, b, w) for a in range(m) for b, w in nb[a].items()
            if a < b]
    heapq.heapify(heap)
    live = m
    while live > 1:
        _, a, b, cut = heapq.heappop(heap)  # a pair has one entry and its delta never changes: the heap's minimum
        if dead[a] or dead[b]:              # over live pairs is the minimum of (delta, a, b)
            continue
        t = len(vol)
        dead[a] = dead[b] = True
        parent[a] = parent[b] = t
        vol.append(vol[a] + vol[b])
        g.append(g[a] + g[b] - 2 * cut)
        cc.append(cut)
        parent.append(-1)
        dead.append(False)
        row = {}
        for x in set(nb[a]) | set(nb[b]):
            if x == a or x == b:
                continue
            c = nb[a].get(x, 0.0) + nb[b].get(x, 0.0)
            nb[x].pop(a, None)
            nb[x].pop(b, None)
            if c != 0:
                row[x] = nb[x][t] = c
                heapq.heappush(heap, (_merge_delta(vol[x], g[x], vol[t], g[t], c, VOL), x, t, c))
        nb[a] = nb[b] = None
        nb.append(row)
        live -= 1
    M = len(vol)
    root = M - 1
    alive = [True] * M
    while True:
        h, depth = [0] * M, [0] * M
        for u in range(M - 1):  # a parent's id is larger than its children's
            if alive[u]:
                h[parent[u]] = max(h[parent[u]], h[u] + 1)
        if h[root] <= 2:
            break
        for u in range(M - 2, -1, -1):
            if alive[u]:
                depth[u] = depth[parent[u]] + 1
        _, u = min((cc[u] * math.log(vol[parent[u]] / vol[u]), u) for u in range(m, M - 1)
                   if alive[u] and depth[u] + h[u] > 2)
        p = parent[u]
        for c in range(u):
            if alive[c] and parent[c] == u:
                parent[c] = p
        cc[p] += cc[u]
        alive[u] = False
    clusters = [[nodes[x] for x in range(m) if parent[x] == u] for u in range(m, M - 1) if alive[u] and parent[u] == root]
    clusters += [[nodes[x]] for x in range(m) if parent[x] == root]
    return clusters


def _host_graph(n: int, src: List[int], dst: List[int], w: Optional[List[float]]) -> Tuple[List[int], int]:
    """(labels, number of clusters) of one graph given by local indices, in float64."""
    adj = [dict() for _ in range(n)]
    for e in range(len(src)):
        i, j = src[e], dst[e]
        if i == j:
            continue
        we = 1.0 if w is None else w[e]
        adj[i][j] = adj[i].get(j, 0.0) + we
        adj[j][i] = adj[j].get(i, 0.0) + we
    for row in adj:
        if not all(math.isfinite(v) and v >= 0 for v in row.values()):
            raise ValueError(_BAD_WEIGHT)
        for j in [j for j, v in row.items() if v == 0]:
            del row[j]  # a zero entry is "not adjacent"
    labels, k, seen = [-1] * n, 0, [False] * n
    for s in range(n):  # components in the order of their smallest node
        if seen[s]:
            continue
        seen[s] = True
        stack, comp = [s], []
        while stack:
            u = stack.pop()
            comp.append(u)
            for v in adj[u]:
                if not seen[v]:
                    seen[v] = True
                    stack.append(v)
        comp.sort()
        for grp in ([comp] if len(comp) == 1 else _host_component(comp, adj)):
            for u in grp:
                labels[u] = k
            k += 1
    return labels, k


def _host_labels(ei: Tensor, ew: Optional[Tensor], batch: Optional[Tensor], n: int, only=None):
    """{graph id: (its nodes, local labels, count)} by the host route; ``only``: the graph ids wanted."""
    ei_h = ei.detach().cpu()
    w_h = None if ew is None else ew.detach().reshape(-1).double().cpu()
    b_h = torch.zeros(n, dtype=torch.long) if batch is None else batch.detach().long().cpu()
    if ei_h.numel() and (int(ei_h.min()) < 0 or int(ei_h.max()) >= n):
        raise ValueError(_BAD_INDEX)
    if w_h is not None and w_h.numel() != ei_h.size(1):
        raise ValueError(f"sep_select: {w_h.numel()} weights for {ei_h.size(1)} edges")
    eg = b_h[ei_h[0]] if ei_h.numel() else torch.zeros(0, dtype=torch.long)
    if ei_h.numel() and bool((eg != b_h[ei_h[1]]).any()):
        raise ValueError(_BAD_INDEX)
    out = {}
    local = torch.zeros(n, dtype=torch.long)
    for gidx in (range(int(b_h.max()) + 1 if n else 0) if only is None else only):
        nodes = (b_h == gidx).nonzero(as_tuple=True)[0]
        if nodes.numel() == 0:
            continue
        local[nodes] = torch.arange(nodes.numel())
        e = (eg == gidx).nonzero(as_tuple=True)[0]
        lab, k = _host_graph(nodes.numel(), local[ei_h[0, e]].tolist(), local[ei_h[1, e]].tolist(),
                             None if w_h is None else w_h[e].tolist())
        out[gidx] = (nodes, torch.tensor(lab, dtype=torch.long), k)
    return out


# ------------------------------------------------------------------------------------------------ select
def sep_select(edge_index, edge_weight: Optional[Tensor] = None, batch: Optional[Tensor] = None,
               num_nodes: Optional[int] = None, *, s_inv_op: str = "transpose", route: Optional[str] = None) -> SelectOutput:
    """Nodes -> depth-1 SEP clusters (reference select/sep_select.py, ``levels=1``).  ``route``: None picks (module
    docstring), ``"host"`` forces the host route, ``"native"`` refuses inputs the kernel does not take.  The result
    carries ``_sep_route``: "native", "host" or "mixed"."""
    if route not in (None, "host", "native"):
        raise ValueError(f"route must be None, 'host' or 'native', got {route!r}")
    ei, ew = connectivity_to_edge_index(edge_index, edge_weight)
    if num_nodes is None:
        num_nodes = int(batch.numel()) if batch is not None else (int(ei.max()) + 1 if ei.numel() else 0)
    n = int(num_nodes)
    if batch is not None and batch.numel() != n:
        raise ValueError(f"Expected batch with {n} nodes, got {batch.numel()}.")
    dev = ei.device
    if ew is not None:
        ew = ew.reshape(-1)
        if not ew.is_floating_point():
            ew = ew.float()
    if n == 0:
        empty = torch.empty(0, dtype=torch.long, device=dev)
        return SelectOutput(cluster_index=empty, num_nodes=0, num_supernodes=0, s_inv_op=s_inv_op, _trusted=True)
    native = ei.is_cuda and (ew is None or ew.dtype == torch.float32) and (batch is None or batch.is_cuda)
    info = None
    if native and batch is not None:
        info = batch_info(batch)
        native = info.is_sorted
    if route == "native" and not native:
        raise ValueError("sep_select: route='native' needs device tensors, float32 (or no) weights and a sorted batch")
    native = native and route != "host"
    cluster = torch.empty(n, dtype=torch.long, device=dev)
    if native:
        limit = K.sep_max_nodes()
        if info is None:
            ptr32 = torch.tensor([0, n], dtype=torch.int32, device=dev)
            gid = torch.zeros(n, dtype=torch.int32, device=dev)
            sizes = [n]
        else:
            ptr32, gid, sizes = info.ptr.to(torch.int32), batch.to(torch.int32), None
        longest = n if info is None else int(info.max_nodes)
        res = K.sep_select(ei, ew, gid, ptr32, n, min(longest, limit))
        st = res["status"]
        if st & K.SEP_BAD_INPUT:
            raise ValueError(_BAD_INDEX)
        if st & K.SEP_BAD_WEIGHT:
            raise ValueError(_BAD_WEIGHT)
        if not st & K.SEP_OVER_LIMIT:
            cluster, total, used = res["cluster_index"], res["total"], "native"
        else:
            # some graphs are past the node limit: theirs come from the host route, and every offset is taken again
            sizes = sizes if sizes is not None else [int(v) for v in info.sizes_host]
            over = [g for g, m in enumerate(sizes) if m > limit]
            host = _host_labels(ei, ew, batch, n, only=over)
            counts = res["counts"].tolist()
            for g in over:
                counts[g] = host[g][2]
            offs, total = [], 0
            for c in counts:
                offs.append(total)
                total += c
            shift = torch.tensor(offs, dtype=torch.long, device=dev) - res["offsets"].long()
            cluster = res["cluster_index"] + shift[gid.long()]
            for g in over:
                nodes, lab, _ = host[g]
                cluster[nodes.to(dev)] = (lab + offs[g]).to(dev)
            used = "mixed" if len(over) < sum(1 for m in sizes if m > 0) else "host"
    else:
        total = 0
        for g, (nodes, lab, k) in sorted(_host_labels(ei, ew, batch, n).items()):
            cluster[nodes.to(dev)] = (lab + total).to(dev)
            total += k
        used = "host"
    so = SelectOutput(cluster_index=cluster, num_nodes=n, num_supernodes=int(total), s_inv_op=s_inv_op, _trusted=True)
    so.__dict__["_no_empty_cluster"] = True  # every id is the rank of a cluster that has its nodes
    so.__dict__["_sep_route"] = used
    return so


class SEPSelect(Select):
    r"""The :math:`\texttt{select}` operator of SEP pooling (reference select/sep_select.py): every node goes to its
    depth-1 cluster of a height-2 coding tree of minimal structural entropy, grown per graph (module docstring, also for
    the deviations from the reference).  ``x`` is an unused placeholder, as in the reference."""

    def __init__(self, s_inv_op: str = "transpose"):
        super().__init__()
        self.s_inv_op = s_inv_op

    def forward(self, x: Optional[Tensor] = None, edge_index=None, edge_weight: Optional[Tensor] = None, *,
                batch: Optional[Tensor] = None, num_nodes: Optional[int] = None, **kwargs) -> SelectOutput:
        return self.multi_level_select(edge_index=edge_index, edge_weight=edge_weight, batch=batch, num_nodes=num_nodes,
                                       levels=1, **kwargs)[0]

    def multi_level_select(self, edge_index=None, edge_weight: Optional[Tensor] = None, *,
                           batch: Optional[Tensor] = None, num_nodes: Optional[int] = None, levels: int = 1,
                           **kwargs) -> List[SelectOutput]:
        if levels < 1:
            raise ValueError(f"'levels' must be >= 1, got {levels}.")
        if levels > 1:
            raise NotImplementedError(_LEVELS_MESSAGE)
        return [sep_select(edge_index, edge_weight, batch, num_nodes, s_inv_op=self.s_inv_op,
                           route=kwargs.get("route"))]

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}()"


# ------------------------------------------------------------------------------------------------ pooler
class SEPPooling(BasePrecoarseningMixin, SRCPooling):
    r"""The SEP pooling operator from `"Structural Entropy Guided Graph Hierarchical Pooling"
    <https://proceedings.mlr.press/v162/wu22b/wu22b.pdf>`_ (Wu et al., ICML 2022; reference poolers/sep.py): select =
    :class:`SEPSelect`, reduce = :class:`~tgp.reduce.BaseReduce`, connect = :class:`~tgp.connect.SparseConnect`, lift =
    :class:`~tgp.lift.BaseLift`.  :meth:`forward` exposes the partition right above the original nodes.

    The selector does not learn: it runs once per dataset under ``cached=True`` or :meth:`precoarsening`.
    :meth:`multi_level_precoarsening` is built for ``levels=1`` only and raises ``NotImplementedError`` beyond (module
    docstring, also for the deviations from the reference)."""

    def __init__(self, lift: str = "precomputed", s_inv_op: str = "transpose", connect_red_op: str = "sum",
                 lift_red_op: str = "sum", cached: bool = False, remove_self_loops: bool = True,
                 degree_norm: bool = True, edge_weight_norm: bool = False):
        super().__init__(
            selector=SEPSelect(s_inv_op=s_inv_op),
            reducer=BaseReduce(),
            lifter=BaseLift(matrix_op=lift, reduce_op=lift_red_op),
            connector=SparseConnect(reduce_op=connect_red_op, remove_self_loops=remove_self_loops,
                                    degree_norm=degree_norm, edge_weight_norm=edge_weight_norm),
            cached=cached)
        self.cached = cached

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None, so: Optional[SelectOutput] = None,
                batch: Optional[Tensor] = None, lifting: bool = False, **kwargs) -> Union[PoolingOutput, Tensor]:
        if lifting:
            return self.lift(x_pool=x, so=so)
        if so is None:
            so = self.select(edge_index=adj, edge_weight=edge_weight, batch=batch, num_nodes=x.size(0))
        fused = self.reduce_connect(x, adj, edge_weight, so, batch)  # batches of small graphs: ONE launch
        if fused is not None:
            x_pool, batch_pool, ei, ew = fused
            return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)
        x_pool, batch_pool = self.reduce(x=x, so=so, batch=batch)
        ei, ew = self.connect(edge_index=adj, so=so, edge_weight=edge_weight, batch_pooled=batch_pool)
        return PoolingOutput(x=x_pool, edge_index=ei, edge_weight=ew, batch=batch_pool, so=so)

    def multi_level_precoarsening(self, levels: int, edge_index=None, edge_weight: Optional[Tensor] = None, *,
                                  batch: Optional[Tensor] = None, num_nodes: Optional[int] = None,
                                  **kwargs) -> List[PoolingOutput]:
        """One SEP pre-coarsening level.  The reference reads deeper levels off one deeper coding tree; the generic
        level-by-level roll-out would build another hierarchy, so ``levels > 1`` is refused."""
        if levels < 1:
            raise ValueError(f"'levels' must be >= 1, got {levels}.")
        if levels > 1:
            raise NotImplementedError(_LEVELS_MESSAGE)
        if edge_index is None:
            raise ValueError("edge_index cannot be None for pre-coarsening.")
        self.clear_cache()
        out = [self.precoarsening(edge_index=edge_index, edge_weight=edge_weight, batch=batch, num_nodes=num_nodes,
                                  **kwargs)]
        self.clear_cache()
        return out

    def extra_repr_args(self) -> dict:
        return {"cached": self.cached}
