"""EigenPooling (Ma et al., KDD 2019; reference poolers/eigenpool.py, select/eigenpool_select.py,
reduce/eigenpool_reduce.py, connect/eigenpool_conn.py, lift/eigenpool_lift.py).

Select partitions every graph into ``k`` clusters and takes, per cluster, the first ``H`` eigenvectors of the Laplacian
of the cluster's induced subgraph.  The reference writes them into a dense pooling matrix ``Theta [n, K H]`` per graph
(column ``h K + c`` = mode ``h`` of cluster ``c``); a row of it has at most ``H`` non-zeros, so this build keeps the
compact form instead -- ``SelectOutput`` extras

    theta_modes [N, H]      node i's entry in mode h of its own cluster
    theta_ptr   [B K + 1]   offsets of the (graph, cluster) groups into theta_perm
    theta_perm  [N]         the nodes by group, ascending node index inside a group

-- and :func:`eigenpool_theta` materialises the reference's matrix (a tensor for one graph, a list for a batch) for
whoever wants it.  Reduce is ``X_pool[g, c, h F + f] = sum_{i in (g, c)} theta_modes[i, h] X[i, f]``, Lift its adjoint,
Connect ``Omega^T A_ext Omega`` with the hard ``Omega = S``.

Routes.  Device float32 inputs take the native kernels of ``csrc/eigenpool.hip``.  Composed from torch
operators on the device, with the same rules: groups of more than ``kernels.eigenpool_max_group_nodes()`` nodes and
adjacencies that are not symmetric (``torch.linalg.eigh`` in float64, lower triangle), float64 inputs, a ``SelectOutput``
that carries the reference's dense or list ``theta`` and no compact extras, and the k-means steps of the labeller.  Host
tensors are refused: there is no CPU fallback.

Labels.  The reference clusters with scikit-learn's ``SpectralClustering`` (k-means with ten unseeded random restarts):
its labels differ from run to run and cannot be reproduced.  The rules that do not depend on chance are kept
(``k >= n``: one cluster per node; an effective ``k`` of 1: one cluster; width ``min(k, n)`` for one graph unless
``fixed_k``, ``k`` for a batch).  Otherwise :class:`EigenPoolSelect` runs a deterministic spectral clustering of its own:
the first ``k`` eigenvectors of the graph's normalised Laplacian scaled by ``D^-1/2`` (the modes kernel with the whole
graph as one group), then k-means with farthest-first initialisation from the highest-degree node (ties to the lower
index) and Lloyd steps until the labels stop changing (at most ``KMEANS_MAX_STEPS``); clusters are numbered by their
lowest member node.  ``labels=`` (a ``[N]`` long tensor of per-graph cluster ids) bypasses the clustering: that is how
the reference's own labels, or any other clustering, are fed in.
"""
from __future__ import annotations

import warnings
from typing import List, Optional, Tuple, Union

import torch
from torch import Tensor

from .. import _native as N
from .. import functions as Fn
from .. import kernels as K
from ..connect import DenseConnect
from ..lift import Lift
from ..reduce.base_reduce import Reduce
from ..select import Select, SelectOutput
from ..src import BasePrecoarseningMixin, DenseSRCPooling, PoolingOutput
from ..utils.ops import (_normalize_pooled_edges, batch_info, build_pooled_batch, connectivity_to_edge_index, is_dense_adj,
                         is_multi_graph_batch, like_input_dtype, postprocess_adj_pool_dense)

KMEANS_MAX_STEPS = 100  # Lloyd steps of the labeller (it stops earlier when the labels repeat)
_TINY = {torch.float64: 4.9406564584124654e-324}  # np.spacing(0) of the adjacency's dtype; fp32 (and half) below
_TINY32 = 1.401298464324817e-45


# ------------------------------------------------------------------------------------------------ modes
def _group_sizes(groups: K.AssignIndex) -> Tensor:
    rp = groups.row_ptr
    return (rp[1:] - rp[:-1]).long()


def _composed_modes(theta: Tensor, todo: List[int], groups: K.AssignIndex, ei: Tensor, ew: Optional[Tensor], gid: Tensor,
                    num_modes: int, normalized: bool, embed: bool, deg: Optional[Tensor]) -> None:
    """The modes of the groups ``todo`` with torch operators on the device (float64 ``torch.linalg.eigh``, which reads
    the lower triangle as numpy's does), written into ``theta`` (and the induced degrees into ``deg``)."""
    if not todo:
        return
    dev, n = theta.device, theta.size(0)
    row, col = ei[0], ei[1]
    g64 = gid.long()
    w = torch.ones(row.numel(), dtype=torch.float32, device=dev) if ew is None else ew.reshape(-1)
    if w.dtype not in (torch.float32, torch.float64):
        w = w.float()
    tiny = _TINY.get(w.dtype, _TINY32)
    # the intra-group edges, by group (edge-list order inside a group)
    intra = (g64[row] == g64[col]).nonzero(as_tuple=True)[0]
    eg = g64[row[intra]]
    order = torch.sort(eg, stable=True)[1]
    intra = intra[order]
    eptr = torch.zeros(groups.num_targets + 1, dtype=torch.long, device=dev)
    eptr[1:] = torch.cumsum(torch.bincount(eg, minlength=groups.num_targets), 0)
    eptr_h, nptr_h = eptr.tolist(), groups.row_ptr.tolist()
    perm = groups.perm.long()
    loc = torch.zeros(n, dtype=torch.long, device=dev)
    for g in todo:
        nodes = perm[nptr_h[g]:nptr_h[g + 1]]
        m = nodes.numel()
        if m == 0:
            continue
        e = intra[eptr_h[g]:eptr_h[g + 1]]
        loc[nodes] = torch.arange(m, device=dev)
        a = torch.zeros(m, m, dtype=w.dtype, device=dev).index_put_((loc[row[e]], loc[col[e]]), w[e], accumulate=True)
        a64 = a.double()
        d = a64.sum(0)
        if deg is not None:
            deg[nodes] = d.to(deg.dtype)
        if m == 1:
            theta[nodes[0], :] = a[0, 0].to(theta.dtype)
            continue
        if normalized:
            dis = 1.0 / torch.sqrt(d + tiny)
            lap = torch.eye(m, dtype=torch.float64, device=dev) - (dis.view(-1, 1) * a64) * dis.view(1, -1)
        else:
            lap = torch.diag(d) - a64
        if not bool(torch.isfinite(lap).all()):
            theta[nodes] = float("nan")  # (eigh refuses non-finite input; the reference's modes are NaN too)
            continue
        _, u = torch.linalg.eigh(lap)
        idx = [min(h, m - 1) for h in range(num_modes)]
        v = u[:, idx]
        v = torch.where(v[0:1] < 0, -v, v)
        if embed:
            v = v * torch.where(d > 0, d.clamp(min=1e-300).rsqrt(), torch.ones_like(d)).view(-1, 1)
        theta[nodes] = v.to(theta.dtype)


def _modes(ei: Tensor, ew: Optional[Tensor], by_src: Optional[K.AssignIndex], gid: Tensor, groups: K.AssignIndex,
           num_modes: int, normalized: bool, embed: bool = False, want_degree: bool = False,
           max_m: Optional[int] = None):
    """theta_modes [N, H] (float32, or float64 for float64 weights) of the groups of ``gid``, by the native kernel where
    it applies and composed for the rest; with ``want_degree`` also the induced degrees [N]."""
    dev = gid.device
    n = gid.numel()
    f64 = ew is not None and ew.dtype == torch.float64
    sizes = _group_sizes(groups)
    limit = K.eigenpool_max_group_nodes()
    if max_m is None:
        max_m = int(sizes.max()) if sizes.numel() else 0
    known_asym = K._adj_symmetric_memo(ei, ew) is False
    deg = None
    if f64 or known_asym or max_m == 0 or ei.size(1) == 0:  # (no edges: every Laplacian is the identity or zero)
        theta = torch.zeros(n, num_modes, dtype=torch.float64 if f64 else torch.float32, device=dev)
        deg = torch.zeros(n, dtype=theta.dtype, device=dev) if want_degree else None
        todo = (sizes > 0).nonzero(as_tuple=True)[0].tolist()
    else:
        if by_src is None:
            by_src = K.edge_group(ei, n)
        out = K.eigenpool_modes(by_src, ei[1], ew, gid, groups, num_modes, min(max_m, limit), normalized, embed,
                                want_degree)
        theta, st = out[0], out[1]
        deg = out[2] if want_degree else None
        if st & K.EIG_ASYMMETRIC:  # which groups the kernel left is not recorded: every group of two or more is redone
            todo = (sizes > 1).nonzero(as_tuple=True)[0].tolist()
        elif st & K.EIG_OVER_LIMIT:
            todo = (sizes > limit).nonzero(as_tuple=True)[0].tolist()
        else:
            todo = []
    _composed_modes(theta, todo, groups, ei, ew, gid, num_modes, normalized, embed, deg)
    return (theta, deg) if want_degree else theta


# ------------------------------------------------------------------------------------------------ labels
def _first_argmax(v: Tensor) -> Tensor:
    """argmax along the last axis, ties (and rows of NaN) to the lowest index."""
    n = v.size(-1)
    mx = v.max(dim=-1, keepdim=True)[0]
    ar = torch.arange(n, device=v.device).expand_as(v)
    return torch.where(v == mx, ar, torch.full_like(ar, n - 1)).min(dim=-1)[0]


def _spectral_labels(ei: Tensor, ew: Optional[Tensor], by_src: Optional[K.AssignIndex], gb: Tensor, sizes: Tensor,
                     ptr: Tensor, k: int) -> Tensor:
    """Per-graph cluster ids [N] in ``0 .. min(k, n_g) - 1``: the rules of the reference's ``_cluster_from_adj`` where
    they decide, the deterministic spectral clustering of the module docstring elsewhere.  Batched over the graphs: the
    only Python loop is the one over the k-means steps."""
    dev, n, B = gb.device, gb.numel(), sizes.numel()
    pos = torch.arange(n, device=dev) - ptr[gb]
    n_of = sizes[gb]
    by_rule = (n_of <= k) | (k <= 1)
    rule_labels = torch.where(n_of <= k, pos, torch.zeros_like(pos)) if k > 1 else torch.zeros_like(pos)
    if bool(by_rule.all()):
        return rule_labels
    graphs = K.build_assign_index(gb, B)
    emb, deg = _modes(ei, ew, by_src, gb.to(torch.int32), graphs, k, True, embed=True, want_degree=True)
    emb, deg = emb.float(), deg.float()
    nmax = int(sizes.max())
    e_pad = torch.zeros(B, nmax, k, dtype=torch.float32, device=dev)
    e_pad[gb, pos] = emb
    valid = torch.zeros(B, nmax, dtype=torch.bool, device=dev)
    valid[gb, pos] = True
    neg = torch.full((B, nmax), float("-inf"), device=dev)
    d_pad = neg.clone()
    d_pad[gb, pos] = deg
    rows = torch.arange(B, device=dev)
    # farthest-first initialisation from the highest-degree node
    first = _first_argmax(d_pad)
    centers = torch.zeros(B, k, k, dtype=torch.float32, device=dev)
    centers[:, 0] = e_pad[rows, first]
    mind = torch.where(valid, ((e_pad - centers[:, 0:1]) ** 2).sum(-1), neg)
    for j in range(1, k):
        nxt = _first_argmax(mind)
        centers[:, j] = e_pad[rows, nxt]
        mind = torch.where(valid, torch.minimum(mind, ((e_pad - centers[:, j:j + 1]) ** 2).sum(-1)), neg)
    lab = None
    for _ in range(KMEANS_MAX_STEPS):
        d2 = ((e_pad.unsqueeze(2) - centers.unsqueeze(1)) ** 2).sum(-1)  # [B, nmax, k]
        new = torch.where(valid, d2.argmin(-1), torch.zeros_like(first).view(-1, 1))
        if lab is not None and torch.equal(new, lab):
            break
        lab = new
        onehot = torch.nn.functional.one_hot(lab, k).to(torch.float32) * valid.unsqueeze(-1)
        cnt = onehot.sum(1)  # [B, k]
        sums = torch.bmm(onehot.transpose(1, 2), e_pad)
        centers = torch.where(cnt.unsqueeze(-1) > 0, sums / cnt.clamp(min=1.0).unsqueeze(-1), centers)
    labels = torch.where(by_rule, rule_labels, lab[gb, pos])
    # clusters numbered by their lowest member node
    low = torch.full((B * k,), n + 1, dtype=torch.long, device=dev)
    low = low.scatter_reduce(0, gb * k + labels, pos, "amin", include_self=True).view(B, k)
    order = torch.sort(low, dim=1, stable=True)[1]
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(k, device=dev).expand(B, k))
    return rank[gb, labels]


# ------------------------------------------------------------------------------------------------ select
def eigenpool_select(edge_index, k: int, edge_weight: Optional[Tensor] = None, batch: Optional[Tensor] = None,
                     num_nodes: Optional[int] = None, fixed_k: bool = False, s_inv_op: str = "transpose",
                     num_modes: int = 5, normalized: bool = True, labels: Optional[Tensor] = None) -> SelectOutput:
    """EigenPool assignments and the compact eigenvector pooling matrix (reference select/eigenpool_select.py:206-380).
    ``so.s`` is the reference's dense one-hot ``[N, K]``; ``so.theta`` is not set (see :func:`eigenpool_theta`)."""
    ei, ew = connectivity_to_edge_index(edge_index, edge_weight)
    inferred = int(ei.max().item()) + 1 if ei.numel() > 0 else 0
    if batch is not None:
        inferred = max(inferred, batch.size(0))
    num_nodes = inferred if num_nodes is None else max(int(num_nodes), inferred)
    if num_nodes == 0:
        raise ValueError("Cannot perform eigenpool selection on empty graph.")
    dev = N.require_device(ei, ew, batch, labels)
    if num_modes < 1:
        raise ValueError(f"num_modes must be at least 1, got {num_modes}")
    if ew is not None:
        ew = ew.reshape(-1)
    n = num_nodes
    multi = is_multi_graph_batch(batch)
    if multi:
        if batch.numel() != n:
            raise ValueError(f"batch names {batch.numel()} nodes, the connectivity {n}")
        info = batch_info(batch)
        if not info.is_sorted:
            raise ValueError("EigenPoolSelect expects the nodes of a batch grouped by graph (a sorted batch vector).")
        gb, sizes, ptr = batch.long(), info.sizes.long(), info.ptr
        width = int(k)
    else:
        gb = torch.zeros(n, dtype=torch.long, device=dev)
        sizes = torch.full((1,), n, dtype=torch.long, device=dev)
        ptr = torch.tensor([0, n], dtype=torch.long, device=dev)
        width = int(k) if fixed_k else max(1, min(int(k), n))
    B = sizes.numel()
    by_src = K.edge_group(ei, n) if ei.size(1) else None
    if labels is None:
        labels = _spectral_labels(ei, ew, by_src, gb, sizes, ptr, int(k))
    else:
        labels = labels.reshape(-1).long()
        if labels.numel() != n:
            raise ValueError(f"labels names {labels.numel()} nodes, the connectivity {n}")
        lo, hi = torch.aminmax(labels)
        if int(lo) < 0 or int(hi) >= width:
            raise ValueError(f"labels must lie in [0, {width}), got [{int(lo)}, {int(hi)}]")
    gid = (gb * width + labels).to(torch.int32)
    groups = K.build_assign_index(gid, B * width)
    max_len = int(_group_sizes(groups).max())  # the longest group: sizes the modes launch and picks the Reduce route
    theta_modes = _modes(ei, ew, by_src, gid, groups, int(num_modes), bool(normalized), max_m=max_len)
    out_dtype = torch.get_default_dtype() if ew is None else ew.dtype
    s = torch.zeros(n, width, dtype=out_dtype, device=dev)
    s.scatter_(1, labels.view(-1, 1), 1.0)
    so = SelectOutput(s=s, s_inv_op=s_inv_op, batch=batch, theta_modes=theta_modes.to(out_dtype),
                      theta_ptr=groups.row_ptr, theta_perm=groups.perm[:n])
    so.__dict__["_eig_cache"] = (so.theta_ptr, groups, gid, max_len)
    return so


def _compact_of(so: SelectOutput, batch: Optional[Tensor]):
    """(theta_modes, groups, gid, longest group) of a SelectOutput with the compact extras, else None.  The index objects
    are cached on ``so`` for exactly the ``theta_ptr`` tensor they were built from (a moved SelectOutput rebuilds them)."""
    tm = so.__dict__.get("theta_modes")
    tp, tperm = so.__dict__.get("theta_ptr"), so.__dict__.get("theta_perm")
    if tm is None or tp is None or tperm is None:
        return None
    hit = so.__dict__.get("_eig_cache")
    if hit is not None and hit[0] is tp and hit[2].device == tm.device:
        return tm, hit[1], hit[2], hit[3]
    n, width = so.s.size(-2), so.s.size(-1)
    G = tp.numel() - 1
    groups = K.AssignIndex(tp.to(torch.int32).contiguous(), tperm.to(torch.int32).contiguous(), n, G)
    labels = so.s.reshape(n, width).argmax(-1)
    if G > width:
        b = batch if batch is not None else so.batch
        gid = (b.long() * width + labels).to(torch.int32)
    else:
        gid = labels.to(torch.int32)
    max_len = int(_group_sizes(groups).max()) if G else 0
    so.__dict__["_eig_cache"] = (tp, groups, gid, max_len)
    return tm, groups, gid, max_len


def eigenpool_theta(so: SelectOutput) -> Union[Tensor, List[Tensor]]:
    """The reference-shaped pooling matrix of a :class:`SelectOutput`: ``Theta [N, K H]`` for one graph, a list of
    per-graph matrices for a multi-graph batch; column ``h K + c`` holds mode ``h`` of cluster ``c``.  A ``SelectOutput``
    that already carries ``theta`` hands it back."""
    if "theta" in so.__dict__ and so.__dict__.get("theta_modes") is None:
        return so.theta
    tm = so.theta_modes
    n, width = so.s.size(-2), so.s.size(-1)
    H = tm.size(1)
    labels = so.s.reshape(n, width).argmax(-1)
    cols = labels.view(-1, 1) + torch.arange(H, device=tm.device).view(1, -1) * width
    theta = torch.zeros(n, width * H, dtype=tm.dtype, device=tm.device).scatter_(1, cols, tm)
    if not is_multi_graph_batch(so.batch):
        return theta
    return list(torch.split(theta, batch_info(so.batch).sizes_host, dim=0))


class EigenPoolSelect(Select):
    r"""The :math:`\texttt{select}` operator of EigenPooling (reference select/eigenpool_select.py:383-467): a hard
    assignment :math:`\mathbf{S} \in \{0,1\}^{N \times K}` and the eigenvector pooling matrix, kept in compact form (see
    the module docstring, also for how the clustering deviates from scikit-learn's).  ``forward`` takes ``fixed_k`` and
    ``labels`` as keywords."""

    is_dense: bool = True

    def __init__(self, k: int, s_inv_op: str = "transpose", num_modes: int = 5, normalized: bool = True):
        super().__init__()
        self.k = k
        self.s_inv_op = s_inv_op
        self.num_modes = num_modes
        self.normalized = normalized

    def forward(self, x: Optional[Tensor] = None, edge_index=None, edge_weight: Optional[Tensor] = None, *,
                batch: Optional[Tensor] = None, num_nodes: Optional[int] = None, **kwargs) -> SelectOutput:
        return eigenpool_select(edge_index=edge_index, k=self.k, edge_weight=edge_weight, batch=batch,
                                num_nodes=num_nodes, fixed_k=bool(kwargs.pop("fixed_k", False)), s_inv_op=self.s_inv_op,
                                num_modes=self.num_modes, normalized=self.normalized, labels=kwargs.pop("labels", None))

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(k={self.k})"


# ------------------------------------------------------------------------------------------------ reduce / lift
def _mode_major_to_blocks(x_pool_raw: Tensor, num_clusters: int) -> Tensor:
    num_modes, feat = x_pool_raw.size(0) // num_clusters, x_pool_raw.size(-1)
    return x_pool_raw.view(num_modes, num_clusters, feat).permute(1, 0, 2).reshape(num_clusters, num_modes * feat)


def _blocks_to_mode_major(x_pool: Tensor, num_clusters: int, num_modes: int) -> Tensor:
    feat = x_pool.size(-1) // num_modes
    return x_pool.reshape(num_clusters, num_modes, feat).permute(1, 0, 2).reshape(num_modes * num_clusters, feat)


def _theta_list(theta, batch: Tensor) -> List[Tensor]:
    if isinstance(theta, (list, tuple)):
        return list(theta)
    return list(torch.split(theta, batch_info(batch).sizes_host, dim=0))


def _matmul(a: Tensor, b: Tensor) -> Tensor:
    return torch.sparse.mm(a, b) if a.is_sparse else a.matmul(b)


class EigenPoolReduce(Reduce):
    r"""The :math:`\texttt{reduce}` operator of EigenPooling (reference reduce/eigenpool_reduce.py):
    :math:`\mathbf{X}_{pool} = \boldsymbol{\Theta}^{\top}\mathbf{X}` per graph, laid out ``[K, H F]``.  With the compact
    extras of :class:`EigenPoolSelect` and device float32 features it is one launch of ``tgp_eigenpool_reduce_f32`` over
    all graphs (every row of ``X`` read once for all modes, nodes added in ascending order, no float atomics), whose
    backward is the Lift kernel.  float64 features, and a ``SelectOutput`` that carries the reference's dense or list
    ``theta`` instead, take the composed form."""

    def __init__(self, num_modes: int = 5, reduce_op: str = "sum"):
        super().__init__()
        self.num_modes = num_modes
        self.reduce_op = reduce_op

    def forward(self, x: Tensor, so: SelectOutput, *, batch: Optional[Tensor] = None, edge_index=None,
                edge_weight: Optional[Tensor] = None, return_batched: bool = False,
                **kwargs) -> Tuple[Tensor, Optional[Tensor]]:
        if batch is None and so.batch is not None:
            batch = so.batch
        N.require_device(x, so.s, batch)
        num_clusters = so.s.size(-1)
        multi = is_multi_graph_batch(batch)
        compact = _compact_of(so, batch)
        if compact is not None:
            tm, groups, gid, max_len = compact
            if x.dtype == torch.float64 or tm.dtype == torch.float64:
                G, H = groups.num_targets, tm.size(1)
                dt = torch.promote_types(x.dtype, tm.dtype)
                prod = tm.to(dt).unsqueeze(2) * x.to(dt).unsqueeze(1)  # [N, H, F]
                x_pool = torch.zeros(G, H, x.size(1), dtype=dt, device=x.device).index_add_(0, gid.long(), prod)
                x_pool = x_pool.view(G, H * x.size(1))
            else:
                x_pool = like_input_dtype(Fn.eigenpool_reduce(x.float(), tm.float(), groups, gid, max_len), x)
            num_graphs = max(groups.num_targets // max(num_clusters, 1), 1)
        elif not multi:
            x_pool = _mode_major_to_blocks(_matmul(so.theta.t(), x), num_clusters)
            num_graphs = 1
        else:
            thetas = _theta_list(so.theta, batch)
            xs = torch.split(x, batch_info(batch).sizes_host, dim=0)
            x_pool = torch.cat([_mode_major_to_blocks(_matmul(t.t(), xb), num_clusters) for t, xb in zip(thetas, xs)], 0)
            num_graphs = len(thetas)
        batch_pool = self.reduce_batch(so, batch)
        if return_batched:
            x_pool = x_pool.view(num_graphs, num_clusters, -1)
        return x_pool, batch_pool

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(num_modes={self.num_modes})"


class EigenPoolLift(Lift):
    r"""The :math:`\texttt{lift}` operator of EigenPooling (reference lift/eigenpool_lift.py):
    :math:`\mathbf{X}_{lift} = \boldsymbol{\Theta}\mathbf{X}_{pool,raw}`.  ``x_pool`` is ``[K, H F]``, ``[B K, H F]``
    or ``[B, K, H F]``.  The native route is ``tgp_eigenpool_lift_f32`` (the adjoint of the Reduce kernel, which is its
    backward); the composed routes are those of :class:`EigenPoolReduce`."""

    def __init__(self, num_modes: int = 5, reduce_op: str = "sum"):
        super().__init__()
        self.num_modes = num_modes
        self.reduce_op = reduce_op

    def forward(self, x_pool: Tensor, so: SelectOutput = None, batch: Optional[Tensor] = None,
                batch_pooled: Optional[Tensor] = None, edge_index=None, edge_weight: Optional[Tensor] = None,
                **kwargs) -> Tensor:
        if batch is None and so.batch is not None:
            batch = so.batch
        N.require_device(x_pool, so.s, batch)
        num_clusters = so.s.size(-1)
        multi = is_multi_graph_batch(batch)
        flat = x_pool.reshape(-1, x_pool.size(-1)) if x_pool.dim() == 3 else x_pool
        compact = _compact_of(so, batch)
        if compact is not None:
            tm, groups, gid, max_len = compact
            if flat.size(0) != groups.num_targets:
                raise ValueError(f"x_pool has {flat.size(0)} rows, the selection {groups.num_targets} supernodes")
            if flat.dtype == torch.float64 or tm.dtype == torch.float64:
                H = tm.size(1)
                dt = torch.promote_types(flat.dtype, tm.dtype)
                rows = flat.to(dt).view(flat.size(0), H, -1)[gid.long()]  # [N, H, F]
                return (tm.to(dt).unsqueeze(2) * rows).sum(1)
            return like_input_dtype(Fn.eigenpool_lift(flat.float(), tm.float(), groups, gid, max_len), x_pool)
        if not multi:
            theta = so.theta
            return _matmul(theta, _blocks_to_mode_major(flat, num_clusters, theta.size(-1) // num_clusters))
        thetas = _theta_list(so.theta, batch)
        pools = torch.split(flat, num_clusters, dim=0)
        return torch.cat([_matmul(t, _blocks_to_mode_major(p, num_clusters, t.size(-1) // num_clusters))
                          for t, p in zip(thetas, pools)], 0)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(num_modes={self.num_modes})"


# ------------------------------------------------------------------------------------------------ connect
class EigenPoolConnect(DenseConnect):
    r"""The :math:`\texttt{connect}` operator of EigenPooling (reference connect/eigenpool_conn.py):
    :math:`\mathbf{A}_{coar} = \boldsymbol{\Omega}^{\top}\mathbf{A}_{ext}\boldsymbol{\Omega}` with the hard
    :math:`\boldsymbol{\Omega} = \texttt{so.s}` and :math:`\mathbf{A}_{ext}` the adjacency without its intra-cluster edges.

    With a hard :math:`\boldsymbol{\Omega}` an edge :math:`i \to j` lands on entry :math:`(c_i, c_j)`, so the
    intra-cluster edges (self-loops among them) reach only the diagonal and the inter-cluster edges only the rest:
    :math:`\boldsymbol{\Omega}^{\top}\mathbf{A}_{ext}\boldsymbol{\Omega}` **is**
    :math:`\boldsymbol{\Omega}^{\top}\mathbf{A}\boldsymbol{\Omega}` **with its diagonal set to zero**.  The sparse route
    therefore needs no kernel of its own: it runs the hard-assignment (one-over-K) Connect on the (graph, cluster) ids
    with self-loop removal always on at the coarse level, before the degree normalisation, and then the reference's
    post-processing -- ``[B, K, K]`` dense output with ``adj_transpose=False`` (eigenpool_conn.py:289-297) or, with
    ``sparse_output``, the block-diagonal ``edge_index`` / ``edge_weight``.  With ``remove_self_loops=False`` the
    diagonal is still zero, as in the reference.  float64 weights are densified with torch operators."""

    def forward(self, edge_index, so: SelectOutput, *, edge_weight: Optional[Tensor] = None,
                batch: Optional[Tensor] = None, batch_pooled: Optional[Tensor] = None, **kwargs):
        omega = self._validate_select_output(so)
        if is_dense_adj(edge_index):  # batched dense inputs: A_ext by masking, then the dense Connect
            s3, adj3 = self._prepare_batched_dense_inputs(omega, edge_index)
            ci = s3.argmax(dim=-1)
            a_ext = adj3 * (ci.unsqueeze(2) != ci.unsqueeze(1)).to(adj3.dtype)
            return super().forward(a_ext, so, edge_weight=None, batch=batch, batch_pooled=batch_pooled)
        ei, ew = connectivity_to_edge_index(edge_index, edge_weight)
        dev = N.require_device(ei, ew, omega, batch)
        if omega.dim() == 3 and omega.size(0) == 1:
            omega = omega.squeeze(0)
        elif omega.dim() != 2:
            raise ValueError("[EigenPoolConnect - unbatched]: SelectOutput.s must have shape "
                             f"[N, K] or [1, N, K], but got {omega.size()}.")
        n, kc = omega.size()
        if batch is None:
            batch = torch.zeros(n, dtype=torch.long, device=dev)
        B = int(batch.max().item()) + 1 if batch.numel() > 0 else 1
        G = B * kc
        gid = batch.long() * kc + omega.argmax(dim=-1)
        if ei.size(1) == 0:
            pe, pw = ei.new_zeros((2, 0)), omega.new_zeros(0)
        else:
            w = torch.ones(ei.size(1), dtype=omega.dtype, device=dev) if ew is None else ew.reshape(-1)
            if w.dtype not in (torch.float32, torch.float64):
                w = w.float()
            if Fn._needs_grad(w) or self.sparse_output:  # (the sparse form also drops |w| <= eps, as the reference does)
                pe, pw = Fn.coalesce_edges(ei, w, gid, G, "sum", True)
            else:
                pe, pw = K.coalesce_edges(ei, w, gid, G, "sum", True, eps_filter=False)
        if not self.sparse_output:
            if pw.dtype == torch.float32:
                ptr = torch.arange(B + 1, dtype=torch.long, device=dev) * kc
                adj = Fn.to_dense_adj(pe, pw, build_pooled_batch(B, kc, dev), ptr, B, kc, False) if pe.size(1) else \
                    torch.zeros(B, kc, kc, dtype=torch.float32, device=dev)
            else:
                adj = torch.zeros(G, kc, dtype=pw.dtype, device=dev).index_put_(
                    (pe[0], pe[1] % kc), pw, accumulate=True).view(B, kc, kc)
            adj = postprocess_adj_pool_dense(adj, self.remove_self_loops, self.degree_norm, False, self.edge_weight_norm)
            return like_input_dtype(adj, omega), None
        if self.edge_weight_norm and batch_pooled is None:
            batch_pooled = build_pooled_batch(B, kc, dev)
        pe, pw = _normalize_pooled_edges(pe, pw, G, self.degree_norm, self.edge_weight_norm, batch_pooled)
        return pe, like_input_dtype(pw, omega)


# ------------------------------------------------------------------------------------------------ pooler
class EigenPooling(BasePrecoarseningMixin, DenseSRCPooling):
    r"""The EigenPooling operator from `"Graph Convolutional Networks with EigenPooling"
    <https://arxiv.org/abs/1904.13107>`_ (Ma et al., KDD 2019; reference poolers/eigenpool.py): select =
    :class:`EigenPoolSelect`, reduce = :class:`EigenPoolReduce`, connect = :class:`EigenPoolConnect`, lift =
    :class:`EigenPoolLift`.  Sparse ``edge_index`` (+ ``edge_weight``, ``batch``) inputs on the device, single graphs and
    multi-graph batches; as in the reference there is no padded ``[B, N, N]`` mode.

    The selector does not learn and runs once per dataset under ``cached=True`` or :meth:`precoarsening`; Reduce,
    Connect and Lift run every step -- which is why the native kernels sit there and in the per-cluster eigenproblems,
    while the k-means steps of the labeller are composed torch operators.

    **Deviation from the reference**: the clusters come from a deterministic spectral clustering, not from
    scikit-learn's randomly restarted one (module docstring); ``forward(..., labels=...)`` feeds in any other
    partition, e.g. the reference's own."""

    def __init__(self, k: int, num_modes: int = 5, normalized: bool = True, cached: bool = False,
                 remove_self_loops: bool = True, degree_norm: bool = True, edge_weight_norm: bool = False,
                 adj_transpose: bool = True, lift: str = "precomputed", s_inv_op: str = "transpose",
                 batched: bool = False, sparse_output: bool = False, cache_preprocessing: bool = False):
        if batched:
            warnings.warn("EigenPooling does not support dense padded batched inputs. "
                          "Use batched=False with a sparse edge_index and batch vector.", UserWarning)
        if lift != "precomputed":
            warnings.warn("EigenPooling ignores the 'lift' argument and always uses "
                          "eigenvector-based lifting.", UserWarning)
        super().__init__(
            selector=EigenPoolSelect(k=k, s_inv_op=s_inv_op, num_modes=num_modes, normalized=normalized),
            reducer=EigenPoolReduce(num_modes=num_modes),
            lifter=EigenPoolLift(num_modes=num_modes),
            connector=EigenPoolConnect(remove_self_loops=remove_self_loops, degree_norm=degree_norm,
                                       adj_transpose=adj_transpose, edge_weight_norm=edge_weight_norm,
                                       sparse_output=sparse_output),
            cached=cached, cache_preprocessing=cache_preprocessing, adj_transpose=adj_transpose, batched=False,
            sparse_output=sparse_output)
        self.k = k
        self.num_modes = num_modes
        self.normalized = normalized
        self.cached = cached
        self.preconnector = EigenPoolConnect(remove_self_loops=remove_self_loops, degree_norm=degree_norm,
                                             edge_weight_norm=edge_weight_norm, sparse_output=True)

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None, so: Optional[SelectOutput] = None,
                mask: Optional[Tensor] = None, batch: Optional[Tensor] = None, batch_pooled: Optional[Tensor] = None,
                lifting: bool = False, **kwargs) -> Union[PoolingOutput, Tensor]:
        if lifting:
            x_pool = x
            if x.dim() == 3:
                B, Kc, F = x.shape
                x_pool = x.reshape(-1, F)
                if batch_pooled is None:
                    batch_pooled = build_pooled_batch(B, Kc, x.device)
            return self.lift(x_pool=x_pool, so=so, batch=batch, batch_pooled=batch_pooled)
        if so is None:
            extra = {"labels": kwargs["labels"]} if kwargs.get("labels") is not None else {}
            so = self.select(edge_index=adj, edge_weight=edge_weight, batch=batch, **extra)
        x_pooled, pooled_batch = self.reduce(x=x, so=so, batch=batch)
        adj_pooled, edge_weight_pooled = self.connect(edge_index=adj, so=so, edge_weight=edge_weight, batch=batch,
                                                      batch_pooled=pooled_batch)
        if not self.sparse_output and pooled_batch is not None and pooled_batch.numel() > 0:
            x_pooled = x_pooled.view(-1, so.s.size(-1), x_pooled.size(-1))
        return PoolingOutput(x=x_pooled, edge_index=adj_pooled, edge_weight=edge_weight_pooled, batch=pooled_batch, so=so)

    def precoarsening(self, edge_index=None, edge_weight: Optional[Tensor] = None, *, batch: Optional[Tensor] = None,
                      num_nodes: Optional[int] = None, **kwargs) -> PoolingOutput:
        """Precompute pooling outputs with a fixed assignment width ``k``."""
        return super().precoarsening(edge_index=edge_index, edge_weight=edge_weight, batch=batch, num_nodes=num_nodes,
                                     fixed_k=True, **kwargs)

    def extra_repr_args(self) -> dict:
        return {"batched": self.batched, "k": self.k, "num_modes": self.num_modes, "normalized": self.normalized,
                "cached": self.cached}
