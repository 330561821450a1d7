"""One-channel graph convolutions: the scorers of :class:`~tgp.poolers.SAGPooling`.

``GraphConv`` and ``SAGEConv`` carry PyG's parameter names (``lin_rel`` / ``lin_root``, ``lin_l`` / ``lin_r``) and
``Linear`` initialisation, so a PyG checkpoint of a SAG layer loads unchanged.  Only what the pooler needs exists:
``out_channels == 1``, ``aggr`` "add" / "sum" / "mean", no edge weights -- anything else raises ``NotImplementedError``
naming the argument.  With one output channel projection and aggregation commute, so device float32 tensors take the
native project-then-aggregate scorer (``tgp.functions.sag_score``: one pass over x, E scalar gathers, no ``E x F`` or
``N x F`` temporary); host tensors and other dtypes take the composed form (gather, ``index_add_``, two ``Linear``s).

``GCNConv`` (any width, ``normalize=False`` only, not in ``__all__``) is the layer of MaxCutPool's score net: it carries
PyG's names (``lin.weight``, ``bias``) and initialisation, and its forward is the composed form of
``tgp.poolers.MaxCutScoreNet``, whose native route reads the parameters directly (``tgp.functions.maxcut_score``).

``PANConv`` (any width) is PyG's path-integral convolution, the layer in front of :class:`~tgp.poolers.PANPooling`: it
returns ``(out, M)`` with ``M`` the maximal-entropy-transition matrix the pooler scores by.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import functions as Fn

_AGGR_MEAN = {"add": False, "sum": False, "mean": True}


def _check(name: str, out_channels: int, aggr: str) -> bool:
    if out_channels != 1:
        raise NotImplementedError(f"{name}: out_channels={out_channels} is not implemented (the pooling scorer has one "
                                  "output channel)")
    if not isinstance(aggr, str) or aggr not in _AGGR_MEAN:
        raise NotImplementedError(f"{name}: aggr={aggr!r} is not implemented (one of 'add', 'sum', 'mean')")
    return _AGGR_MEAN[aggr]


class _OneChannelConv(torch.nn.Module):
    """lin_nb(aggr_{j -> i} x_j) + lin_self(x_i); the subclasses name the two ``Linear``s as PyG does."""

    _nb: str
    _self: Optional[str]

    def __init__(self, in_channels: int, out_channels: int, aggr: str, root: bool, bias: bool):
        super().__init__()
        self._mean = _check(type(self).__name__, out_channels, aggr)
        self.in_channels, self.out_channels, self.aggr = in_channels, out_channels, aggr
        setattr(self, self._nb, torch.nn.Linear(in_channels, out_channels, bias=bias))
        if root:
            setattr(self, self._self, torch.nn.Linear(in_channels, out_channels, bias=False))

    def _linears(self):
        return getattr(self, self._nb), getattr(self, self._self, None)

    def reset_parameters(self):
        for lin in self._linears():
            if lin is not None:
                lin.reset_parameters()

    def score(self, x: Tensor, edge_index: Tensor, use_tanh: bool = False) -> Optional[Tensor]:
        """act(forward(x, edge_index)) as a vector [N] from the native scorer, or None when the inputs are not its case
        (host tensors, another dtype, non-tensor connectivity)."""
        nb, root = self._linears()
        if not (isinstance(edge_index, Tensor) and not edge_index.is_sparse and edge_index.dim() == 2
                and edge_index.size(0) == 2 and x.is_cuda and edge_index.is_cuda and x.dim() == 2
                and x.dtype == torch.float32 and nb.weight.dtype == torch.float32 and x.size(0) > 0
                and x.size(1) == self.in_channels):
            return None
        return Fn.sag_score(x, edge_index, nb.weight, None if root is None else root.weight, nb.bias, self._mean,
                            use_tanh)

    def forward(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None) -> Tensor:
        if edge_weight is not None:
            raise NotImplementedError(f"{type(self).__name__}: edge_weight is not implemented (SAGPooling scores without "
                                      "edge weights)")
        x = x.view(-1, 1) if x.dim() == 1 else x
        native = self.score(x, edge_index)
        if native is not None:
            return native.view(-1, 1)
        if not isinstance(edge_index, Tensor) or edge_index.is_sparse:
            from .utils.ops import connectivity_to_edge_index
            edge_index, _ = connectivity_to_edge_index(edge_index, None)
        nb, root = self._linears()
        src, dst = edge_index[0], edge_index[1]
        agg = torch.zeros_like(x).index_add_(0, dst, x[src])
        if self._mean:
            deg = torch.zeros(x.size(0), dtype=x.dtype, device=x.device).index_add_(
                0, dst, torch.ones(dst.numel(), dtype=x.dtype, device=x.device))
            agg = agg / deg.clamp(min=1).view(-1, 1)
        out = nb(agg)
        return out if root is None else out + root(x)

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, aggr={self.aggr}"


class GraphConv(_OneChannelConv):
    r"""PyG's ``GraphConv`` (Morris et al. 2019) at one output channel, without edge weights:
    :math:`\mathbf{W}_1 \mathbf{x}_i + \mathbf{W}_2 \sum_{j \to i} \mathbf{x}_j`.  Parameters ``lin_rel.weight`` [1,F],
    ``lin_rel.bias`` [1], ``lin_root.weight`` [1,F]."""

    _nb, _self = "lin_rel", "lin_root"

    def __init__(self, in_channels: int, out_channels: int, aggr: str = "add", bias: bool = True):
        super().__init__(in_channels, out_channels, aggr, True, bias)


class SAGEConv(_OneChannelConv):
    r"""PyG's ``SAGEConv`` (Hamilton et al. 2017) at one output channel:
    :math:`\mathbf{W}_1 \mathrm{mean}_{j \to i} \mathbf{x}_j + \mathbf{W}_2 \mathbf{x}_i`.  Parameters ``lin_l.weight``
    [1,F], ``lin_l.bias`` [1], ``lin_r.weight`` [1,F] (absent with ``root_weight=False``)."""

    _nb, _self = "lin_l", "lin_r"

    def __init__(self, in_channels: int, out_channels: int, aggr: str = "mean", root_weight: bool = True,
                 bias: bool = True):
        super().__init__(in_channels, out_channels, aggr, bool(root_weight), bias)
        self.root_weight = bool(root_weight)


class GCNConv(torch.nn.Module):
    r"""PyG's ``GCNConv`` as :class:`~tgp.poolers.MaxCutScoreNet` uses it: ``normalize=False``, so
    :math:`\mathbf{x}'_i = \sum_{j \to i} w_{ji} \mathbf{W} \mathbf{x}_j + \mathbf{b}` on the list as given (the caller
    brings the propagation matrix).  Parameters ``lin.weight`` [out, in] (glorot) and ``bias`` [out] (zeros), PyG's names.
    The score net's native route reads these parameters and never calls this forward; this is the composed form."""

    def __init__(self, in_channels: int, out_channels: int, improved: bool = False, cached: bool = False,
                 add_self_loops: Optional[bool] = None, normalize: bool = True, bias: bool = True):
        super().__init__()
        if normalize:
            raise NotImplementedError("GCNConv: normalize=True is not implemented (the MaxCut score net brings its own "
                                      "propagation matrix)")
        if improved or add_self_loops:
            raise NotImplementedError("GCNConv: improved / add_self_loops are not implemented (they belong to "
                                      "normalize=True)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.lin.weight)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None) -> Tensor:
        if not isinstance(edge_index, Tensor) or edge_index.is_sparse:
            from .utils.ops import connectivity_to_edge_index
            edge_index, edge_weight = connectivity_to_edge_index(edge_index, edge_weight)
        z = self.lin(x)
        msg = z[edge_index[0]]
        if edge_weight is not None:
            msg = msg * edge_weight.view(-1, 1).to(msg.dtype)
        out = torch.zeros_like(z).index_add_(0, edge_index[1], msg)
        return out if self.bias is None else out + self.bias

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}"


def pan_met_composed(edge_index: Tensor, weight: Tensor, num_nodes: int):
    """The MET matrix composed from torch operators, any device and float dtype: ``(index [2, nnz], values [nnz])``
    row-major sorted and coalesced, the same pattern in the same order as the kernel's.  ``tmp_n`` is kept as a COO list;
    the product with ``A_t`` expands every entry ``(r, k)`` by the edges ``j -> k`` (the by-destination group of ``k``)
    and merges equal ``(r, j)``; the ``L + 1`` partial lists are then concatenated and merged once more -- PyG's scheme.
    The pattern is structural (nothing is pruned by value), ``deg`` counts stored entries.  Differentiable in
    ``weight`` through torch's own autograd."""
    n, dev, dtype = int(num_nodes), edge_index.device, weight.dtype
    src, dst = edge_index[0].long(), edge_index[1].long()
    src_by_dst = src[torch.argsort(dst, stable=True)]
    indeg = torch.bincount(dst, minlength=n)
    first = torch.cumsum(indeg, 0) - indeg
    ar = torch.arange(n, device=dev)
    rows, cols, vals = ar, ar, weight[0].expand(n)
    keys, terms = [ar * n + ar], [vals]
    for step in range(1, weight.numel()):
        cnt = indeg[cols]
        rep = torch.repeat_interleave(torch.arange(cols.numel(), device=dev), cnt)
        within = torch.arange(rep.numel(), device=dev) - (torch.cumsum(cnt, 0) - cnt)[rep]
        key, inv = torch.unique(rows[rep] * n + src_by_dst[first[cols[rep]] + within], return_inverse=True)
        vals = weight[step] * torch.zeros(key.numel(), dtype=dtype, device=dev).index_add(0, inv, vals[rep])
        rows, cols = torch.div(key, n, rounding_mode="floor"), key % n
        keys.append(key)
        terms.append(vals)
    key, inv = torch.unique(torch.cat(keys), return_inverse=True)
    s = torch.zeros(key.numel(), dtype=dtype, device=dev).index_add(0, inv, torch.cat(terms))
    rows, cols = torch.div(key, n, rounding_mode="floor"), key % n
    dinv = torch.bincount(rows, minlength=n).to(dtype).pow(-0.5)
    dinv = torch.where(torch.isinf(dinv), torch.zeros_like(dinv), dinv)
    return torch.stack([rows, cols]), (dinv[cols] * s) * dinv[rows]


class PANConv(torch.nn.Module):
    r"""PyG's ``PANConv`` (Ma et al., NeurIPS 2020): :math:`\mathbf{X}' = \mathbf{M}\mathbf{X}\mathbf{W}` with the
    maximal-entropy-transition matrix :math:`\mathbf{M} = \mathbf{D}^{-1/2} \sum_{n=0}^{L} c_n \mathbf{A}_t^n
    \mathbf{D}^{-1/2}`, :math:`c_n = \prod_{i \le n}` ``weight[i]``.  Parameters ``lin.weight`` [out, in], ``lin.bias``
    [out] and ``weight`` [L + 1] (reset to 0.5), PyG's names.

    ``forward(x, edge_index, batch=None) -> (out, M)``.  ``A_t[dst, src]`` counts the occurrences of the edge ``src ->
    dst`` (edge values are ignored, duplicates count, self-loops stay); a sparse ``edge_index`` is read as ``A_t`` itself
    (row = target), as PyG reads an ``adj_t``.  The stored pattern of ``M`` is structural -- ``(i, j)`` is kept iff a
    walk of at most ``L`` edges joins them, whatever the value -- and ``D`` counts the stored entries of a row.  ``M``
    comes back as a coalesced torch sparse COO tensor ``[N, N]`` with row = target; it is a
    ``torch_sparse.SparseTensor`` only when that package is importable and the input was one (this build does not
    depend on it).

    ``batch`` tells the native route where the graphs are; without it the whole input is one graph.  Device float32
    inputs whose nodes are grouped by graph, with every edge inside one graph and no graph beyond
    ``kernels.pan_max_graph_nodes()`` nodes, take the row kernels of ``csrc/pan.hip`` (no sparse-sparse product, no
    sort); larger graphs, float64, edges between graphs and host tensors take :func:`pan_met_composed`."""

    def __init__(self, in_channels: int, out_channels: int, filter_size: int, **kwargs):
        super().__init__()
        if kwargs.pop("aggr", "add") != "add" or kwargs:
            raise NotImplementedError(f"PANConv: only aggr='add' and no further arguments are implemented, got {kwargs}")
        if int(filter_size) < 0:
            raise ValueError(f"PANConv: filter_size must not be negative, got {filter_size}")
        self.in_channels, self.out_channels, self.filter_size = in_channels, out_channels, int(filter_size)
        self.lin = torch.nn.Linear(in_channels, out_channels)
        self.weight = torch.nn.Parameter(torch.empty(self.filter_size + 1))
        self.reset_parameters()

    def reset_parameters(self):
        self.lin.reset_parameters()
        self.weight.data.fill_(0.5)

    def met(self, edge_index: Tensor, num_nodes: int, batch: Optional[Tensor] = None):
        """The MET record of ``edge_index`` [2, E]: a ``kernels.PanMet`` (``index``, ``values`` tracked back to
        ``weight``, ``row_ptr``) from the native route, or from the composed form (``frame`` None)."""
        from . import kernels as K
        from .utils.ops import batch_info
        n, dev = int(num_nodes), edge_index.device
        graph_ptr = gid = longest = None
        if edge_index.is_cuda and self.weight.is_cuda and n > 0:
            if batch is None:
                graph_ptr, longest = K.pan_one_graph_ptr(n, dev), n
            elif batch.numel() == n:
                info = batch_info(batch)
                if info.is_sorted:
                    facts = info.memo.get("pan")
                    if facts is None:
                        facts = info.memo["pan"] = (info.ptr.to(torch.int32), batch.to(torch.int32))
                    (graph_ptr, gid), longest = facts, info.max_nodes
        if K.pan_route(edge_index, self.weight, n, graph_ptr, longest) == "native":
            met = Fn.pan_met(edge_index, self.weight, n, gid, graph_ptr, longest)
            if met is not None:
                return met
        index, values = pan_met_composed(edge_index, self.weight, n)
        row_ptr = None
        if index.is_cuda and values.dtype == torch.float32:
            row_ptr = K.rowptr_from_sorted(index[0], n, torch.empty(n + 1, dtype=torch.int32, device=dev))
        return K.PanMet(index, values, row_ptr, n)

    def forward(self, x: Tensor, edge_index, batch: Optional[Tensor] = None):
        from . import kernels as K
        from .imports import is_sparsetensor
        was_sparsetensor = is_sparsetensor(edge_index)
        if not isinstance(edge_index, Tensor) or edge_index.layout != torch.strided:
            from .utils.ops import connectivity_to_edge_index
            if isinstance(edge_index, Tensor) and edge_index.layout != torch.sparse_coo:
                edge_index = edge_index.to_sparse_coo()
            edge_index, _ = connectivity_to_edge_index(edge_index, None)
            edge_index = edge_index.flip(0)  # (a sparse input is A_t: its rows are the targets)
        n = x.size(0)
        met = self.met(edge_index, n, batch)
        if met.row_ptr is not None and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2:
            out = Fn.linear(Fn.pan_spmm(met, x), self.lin.weight, self.lin.bias)
        else:
            out = self.lin(torch.zeros_like(x).index_add(0, met.index[0], met.values.view(-1, 1) * x[met.index[1]]))
        m = torch.sparse_coo_tensor(met.index, met.values, (n, n), is_coalesced=True)
        if met.row_ptr is not None:
            K.pan_remember(m, met)
        if was_sparsetensor:  # pragma: no cover  (torch_sparse is not a dependency of this build)
            from torch_sparse import SparseTensor
            m = SparseTensor(row=met.index[0], col=met.index[1], value=met.values, sparse_sizes=(n, n), is_sorted=True)
        return out, m

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, filter_size={self.filter_size}"


__all__ = ["GraphConv", "SAGEConv"]  # (SAGPooling's scorers; GCNConv and PANConv are imported by name)
