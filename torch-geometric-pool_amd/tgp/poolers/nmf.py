"""NMF pooling (Bacciu and Di Sotto, AIIA 2019; reference poolers/nmf.py, select/nmf_select.py).

Select factorises every graph's clamped dense adjacency, ``A ~ W H`` with ``ka = max(1, min(k, n))`` components, and
returns ``S = softmax(H^T)``; Reduce, Connect and Lift are the existing dense operators on the un-padded ``S [N, K]``.
The reference loops over the graphs in Python, copies each adjacency to the host and calls scikit-learn's
``non_negative_factorization(adj, n_components=ka, init="random", max_iter=5000)``: the coordinate-descent solver
(``shuffle=False``, ``tol=1e-4``, no regularisation).  Here the same iteration runs on the device.

Routes.  Device float32 inputs whose graphs have at most ``kernels.nmf_max_nodes()`` nodes, with ``k`` at
most ``kernels.nmf_max_k()``, take ``tgp_nmf_factorize_f32``: one workgroup per graph, all graphs in one launch, one host
wait per call (the status word).  Graphs past the node limit, a ``k`` past its limit and float64 weights take the same
algorithm composed from torch operators on the device, graph by graph, with the same init; a batch may mix both.  Host
tensors are refused: there is no CPU fallback.

Init.  The reference's init is random and unseeded: its output differs from run to run and cannot be reproduced.  The
rules that do not depend on chance are kept (no rows for an empty graph, the identity for ``n > 1 and ka >= n``, a
column of ones for ``ka == 1``, the widths).  Otherwise the default init is a pure function of ``(seed, factor, node
index inside the graph, component)``: a 32-bit integer hash mixed down to a uniform ``u`` in ``(0, 1]``, the entry being
``avg * 2u`` with scikit-learn's ``avg = sqrt(mean(A) / ka)`` (its scale, mean ``avg``).  It does not depend on the
graph's id or on where its nodes stand in the batch.  ``init=(W0, H0^T)`` (both ``[N, K]``, node-major, non-negative,
columns ``>= ka`` ignored) replaces it: that is how scikit-learn's own init, or any other, is fed in.
"""
from __future__ import annotations

import warnings
from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from .. import _native as N
from .. import kernels as K
from ..connect import DenseConnect
from ..lift import BaseLift
from ..reduce import BaseReduce
from ..select import Select, SelectOutput
from ..src import BasePrecoarseningMixin, DenseSRCPooling, PoolingOutput
from ..utils.ops import batch_info, connectivity_to_edge_index, is_multi_graph_batch

_M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ composed route
def _hash_uniform(seed: int, which: int, n: int, ka: int, dev) -> Tensor:
    """u [n, ka] in (0, 1] (float64, exact): ``nmf_uniform`` of csrc/nmf.hip with int64 operations masked to 32 bits."""
    i = torch.arange(n, dtype=torch.int64, device=dev).view(-1, 1)
    t = torch.arange(ka, dtype=torch.int64, device=dev).view(1, -1)
    base = (((int(seed) & _M32) * 0x9E3779B9) + (int(which) & _M32) * 0x85EBCA6B + 0x165667B1) & _M32
    h = (base + ((i * 0xC2B2AE35) & _M32) + ((t * 0x27D4EB2F) & _M32)) & _M32
    h = h ^ (h >> 16)
    h = (h * 0x7FEB352D) & _M32
    h = h ^ (h >> 15)
    h = (h * 0x846CA68B) & _M32
    h = h ^ (h >> 16)
    return ((h >> 8) + 1).to(torch.float64) / 16777216.0


def _half_sweep(a: Tensor, u: Tensor, f: Tensor) -> Tensor:
    """One coordinate-descent pass over the rows of ``u`` [n, ka] against ``a ~ u f^T`` (in place); the violation as a
    device scalar (float64)."""
    gram = f.t() @ f
    prod = a @ f
    hess = torch.diagonal(gram)
    safe = torch.where(hess != 0, hess, torch.ones_like(hess))
    viol = torch.zeros((), dtype=torch.float64, device=a.device)
    for t in range(u.size(1)):
        grad = -prod[:, t] + u @ gram[t]
        ut = u[:, t].clone()
        pg = torch.where(ut == 0, grad.clamp(max=0), grad)
        viol = viol + pg.abs().double().sum()
        u[:, t] = torch.where(hess[t] != 0, (ut - grad / safe[t]).clamp(min=0), ut)
    return viol


def _composed_factorize(a: Tensor, w0: Tensor, h0t: Tensor, tol: float, max_iter: int):
    """(W, H^T, iterations, last ratio) of the solver on the non-negative ``a`` [n, n] with torch operators on the
    device, in ``a``'s dtype.  One host read per iteration (the convergence test): the route of the few graphs the
    kernel does not take."""
    w, ht = w0.clone(), h0t.clone()
    at = a.t().contiguous()
    vinit, it, ratio = 0.0, 0, 0.0
    for it in range(1, int(max_iter) + 1):
        viol = float(_half_sweep(a, w, ht) + _half_sweep(at, ht, w))
        if it == 1:
            vinit = viol
        if vinit == 0:
            ratio = 0.0
            break
        ratio = viol / vinit
        if ratio <= tol:
            break
    return w, ht, it, ratio


def _composed_graph(ei: Tensor, w: Tensor, gb: Tensor, g: int, lo: int, hi: int, ka: int, seed: int, tol: float,
                    max_iter: int, init) -> Tuple[Tensor, Tensor, Tensor, int, float]:
    dev = ei.device
    m = hi - lo
    e = (gb[ei[0]] == g).nonzero(as_tuple=True)[0]
    r, c = ei[0, e] - lo, ei[1, e] - lo
    if e.numel() and bool(((c < 0) | (c >= m)).any()):
        raise ValueError("nmf_select: an edge whose endpoints lie in two graphs")
    a = torch.zeros(m, m, dtype=w.dtype, device=dev).index_put_((r, c), w[e], accumulate=True).clamp(min=0)
    if not bool(torch.isfinite(a).all()):
        raise ValueError("nmf_select: the adjacency contains NaN or infinity")
    if init is None:
        avg = torch.sqrt(a.mean() / ka)
        w0 = avg * (2.0 * _hash_uniform(seed, 0, m, ka, dev)).to(a.dtype)
        h0t = avg * (2.0 * _hash_uniform(seed, 1, m, ka, dev)).to(a.dtype)
    else:
        w0, h0t = init[0][lo:hi, :ka].to(a.dtype), init[1][lo:hi, :ka].to(a.dtype)
    wf, ht, it, ratio = _composed_factorize(a, w0, h0t, tol, max_iter)
    return torch.softmax(ht, dim=-1), wf, ht, it, ratio


# ------------------------------------------------------------------------------------------------ select
def nmf_select(edge_index, k: int, edge_weight: Optional[Tensor] = None, batch: Optional[Tensor] = None,
               num_nodes: Optional[int] = None, *, fixed_k: bool = False, seed: int = 0, tol: float = 1e-4,
               max_iter: int = 5000, init: Optional[Tuple[Tensor, Tensor]] = None, return_factors: bool = False,
               s_inv_op: str = "transpose"):
    """NMF assignments (reference select/nmf_select.py:120-223): ``so.s`` is ``[N, ka]`` for one graph, ``[N, k]`` with
    ``fixed_k`` or for a multi-graph batch (zero columns behind a graph's ``ka``).  With ``return_factors`` the result is
    ``(so, {"w": [N, k], "ht": [N, k], "iters": [B] int32, "ratio": [B]})``: the raw factors (zeros where nothing is
    factorised), the iteration every factorised graph stopped at and its last violation ratio."""
    ei, ew = connectivity_to_edge_index(edge_index, edge_weight)
    Kc = int(k)
    if Kc < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    if int(max_iter) < 1 or not float(tol) >= 0.0:
        raise ValueError(f"max_iter must be at least 1 and tol non-negative, got {max_iter} and {tol}")
    dev = N.require_device(ei, ew, batch, *(init if init is not None else ()))
    inferred = int(ei.max().item()) + 1 if ei.numel() > 0 else 0
    if batch is not None:
        inferred = max(inferred, batch.size(0))
    n = inferred if num_nodes is None else max(int(num_nodes), inferred)
    if ew is not None:
        ew = ew.reshape(-1)
        if ew.dtype not in (torch.float32, torch.float64):
            ew = ew.float()
    out_dtype = torch.get_default_dtype() if ew is None else ew.dtype
    f64 = out_dtype == torch.float64
    multi = is_multi_graph_batch(batch)
    if multi:
        if batch.numel() != n:
            raise ValueError(f"batch names {batch.numel()} nodes, the connectivity {n}")
        info = batch_info(batch)
        if not info.is_sorted:
            raise ValueError("NMFSelect expects the nodes of a batch grouped by graph (a sorted batch vector).")
        gb, sizes = batch.long(), [int(v) for v in info.sizes_host]
        ptr32 = info.ptr.to(torch.int32)
        width = Kc
    else:
        gb, sizes = torch.zeros(n, dtype=torch.long, device=dev), [n]
        ptr32 = torch.tensor([0, n], dtype=torch.int32, device=dev)
        width = Kc if fixed_k else max(1, min(Kc, n))
    B = len(sizes)
    if init is not None and (tuple(init[0].shape) != (n, Kc) or tuple(init[1].shape) != (n, Kc)):
        raise ValueError(f"init is (W0, H0^T), both [{n}, {Kc}] node-major")
    if n == 0:
        so = SelectOutput(s=torch.zeros(0, Kc if (multi or fixed_k) else 0, dtype=out_dtype, device=dev),
                          s_inv_op=s_inv_op, batch=batch)
        empty = {"w": torch.zeros(0, Kc, dtype=out_dtype, device=dev), "ht": torch.zeros(0, Kc, dtype=out_dtype, device=dev),
                 "iters": torch.zeros(B, dtype=torch.int32, device=dev), "ratio": torch.zeros(B, device=dev)}
        return (so, empty) if return_factors else so
    max_n, max_k = K.nmf_max_nodes(), K.nmf_max_k()
    factorised = [g for g, m in enumerate(sizes) if 1 < Kc < m]
    native = not f64 and Kc <= max_k
    if native:
        todo = [g for g in factorised if sizes[g] > max_n]
        by_src = K.sag_edge_group(ei, n, by_destination=False)  # (remembered per edge_index tensor)
        gid = gb.to(torch.int32)
        # the inverted index of a sorted batch vector: its CSR offsets and the identity (what tgp_assign_index_build gives)
        graphs = K.AssignIndex(ptr32, torch.arange(n, dtype=torch.int32, device=dev), n, B)
        out = K.nmf_factorize(by_src, ei[1], ew, gid, graphs, Kc, width, min(max(sizes), max_n), seed, tol, max_iter, init,
                              return_factors)
        st = out["status"]
        if st & K.NMF_BAD_INPUT:
            raise ValueError("nmf_select: an index outside its table (an edge endpoint or edge position out of range, a "
                             "node outside its graph, or an edge whose endpoints lie in two graphs); nothing out of "
                             "range was read")
        if st & K.NMF_NON_FINITE:
            raise ValueError("nmf_select: the adjacency contains NaN or infinity")
        s = out["s"]
        wf, htf = (out["w"], out["ht"]) if return_factors else (None, None)
        iters, ratio = out["iters"], out["ratio"]
        # a graph past the node limit that needs no factorisation was flagged too: it is written below
        special = [g for g, m in enumerate(sizes) if m > max_n and g not in todo]
    else:
        todo, special = factorised, [g for g in range(B) if g not in factorised]
        s = torch.zeros(n, width, dtype=out_dtype, device=dev)
        wf = torch.zeros(n, Kc, dtype=out_dtype, device=dev) if return_factors else None
        htf = torch.zeros(n, Kc, dtype=out_dtype, device=dev) if return_factors else None
        iters, ratio = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.float32, device=dev)
    if todo or special:
        ptr = [0]
        for m in sizes:
            ptr.append(ptr[-1] + m)
        w = torch.ones(ei.size(1), dtype=out_dtype, device=dev) if ew is None else ew
        for g in special:
            lo, hi = ptr[g], ptr[g + 1]
            m = hi - lo
            if m > 1 and Kc >= m:
                s[lo:hi, :m] = torch.eye(m, dtype=s.dtype, device=dev)
            elif m > 0:
                s[lo:hi, 0] = 1.0
        for g in todo:
            lo, hi = ptr[g], ptr[g + 1]
            sg, wg, hg, it, rt = _composed_graph(ei, w, gb, g, lo, hi, Kc, seed, float(tol), int(max_iter), init)
            s[lo:hi, :Kc] = sg.to(s.dtype)
            iters[g], ratio[g] = it, rt
            if return_factors:
                wf[lo:hi], htf[lo:hi] = wg.to(wf.dtype), hg.to(htf.dtype)
    so = SelectOutput(s=s.to(out_dtype), s_inv_op=s_inv_op, batch=batch)
    if return_factors:
        return so, {"w": wf, "ht": htf, "iters": iters, "ratio": ratio}
    return so


class NMFSelect(Select):
    r"""The :math:`\texttt{select}` operator of NMF pooling (reference select/nmf_select.py): the factorisation
    :math:`\mathbf{A} \approx \mathbf{W}\mathbf{H}` per graph and :math:`\mathbf{S} = \mathrm{softmax}(\mathbf{H}^\top)`
    (see the module docstring, also for how the init deviates from scikit-learn's unseeded one).  ``seed``, ``tol`` and
    ``max_iter`` are this build's; ``forward`` also takes ``init=(W0, H0^T)`` as a keyword."""

    is_dense: bool = True

    def __init__(self, k: int, s_inv_op: str = "transpose", *, seed: int = 0, tol: float = 1e-4, max_iter: int = 5000):
        super().__init__()
        self.k = k
        self.s_inv_op = s_inv_op
        self.seed = seed
        self.tol = tol
        self.max_iter = max_iter

    def forward(self, edge_index, edge_weight: Optional[Tensor] = None, *, batch: Optional[Tensor] = None,
                num_nodes: Optional[int] = None, fixed_k: bool = False, **kwargs) -> SelectOutput:
        return nmf_select(edge_index, self.k, edge_weight, batch, num_nodes, fixed_k=bool(fixed_k), seed=self.seed,
                          tol=self.tol, max_iter=self.max_iter, init=kwargs.pop("init", None), s_inv_op=self.s_inv_op)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(k={self.k}, s_inv_op={self.s_inv_op})"


# ------------------------------------------------------------------------------------------------ pooler
class NMFPooling(BasePrecoarseningMixin, DenseSRCPooling):
    r"""The NMF pooling operator from `"A Non-Negative Factorization approach to node pooling in Graph Convolutional
    Neural Networks" <https://arxiv.org/abs/1909.03287>`_ (Bacciu and Di Sotto, AIIA 2019; reference poolers/nmf.py):
    select = :class:`NMFSelect`, reduce = :class:`~tgp.reduce.BaseReduce`, connect = :class:`~tgp.connect.DenseConnect`,
    lift = :class:`~tgp.lift.BaseLift`.  Sparse ``edge_index`` (+ ``edge_weight``, ``batch``) inputs on the device,
    single graphs and multi-graph batches; as in the reference there is no padded ``[B, N, N]`` mode.

    The selector does not learn: it runs once per dataset under ``cached=True`` or :meth:`precoarsening`.

    **Deviation from the reference**: the factorisation starts from a deterministic seeded init, not from scikit-learn's
    unseeded random one (module docstring); ``seed``, ``tol`` and ``max_iter`` are keyword-only extras."""

    def __init__(self, k: int, cached: bool = False, remove_self_loops: bool = True, degree_norm: bool = True,
                 edge_weight_norm: bool = False, adj_transpose: bool = True, lift: str = "precomputed",
                 s_inv_op: str = "transpose", batched: bool = False, sparse_output: bool = False,
                 cache_preprocessing: bool = False, *, seed: int = 0, tol: float = 1e-4, max_iter: int = 5000):
        if batched:
            warnings.warn("NMFPooling does not support dense padded batched inputs. "
                          "Use sparse edge_index with a batch vector.", UserWarning)
        super().__init__(
            selector=NMFSelect(k=k, s_inv_op=s_inv_op, seed=seed, tol=tol, max_iter=max_iter),
            reducer=BaseReduce(),
            lifter=BaseLift(matrix_op=lift),
            connector=DenseConnect(remove_self_loops=remove_self_loops, degree_norm=degree_norm,
                                   adj_transpose=adj_transpose, edge_weight_norm=edge_weight_norm,
                                   sparse_output=sparse_output),
            cached=cached, cache_preprocessing=cache_preprocessing, adj_transpose=adj_transpose, batched=False,
            sparse_output=sparse_output)
        self.cached = cached
        # the connector of the precoarsening step (always sparse output)
        self.preconnector = DenseConnect(remove_self_loops=remove_self_loops, degree_norm=degree_norm,
                                         edge_weight_norm=edge_weight_norm, sparse_output=True)

    def forward(self, x: Tensor, adj=None, edge_weight: Optional[Tensor] = None, so: Optional[SelectOutput] = None,
                mask: Optional[Tensor] = None, batch: Optional[Tensor] = None, batch_pooled: Optional[Tensor] = None,
                lifting: bool = False, **kwargs) -> Union[PoolingOutput, Tensor]:
        if lifting:
            return self.lift(x_pool=x, so=so, batch=batch, batch_pooled=batch_pooled)
        if so is None:
            so = self.select(edge_index=adj, edge_weight=edge_weight, batch=batch, num_nodes=x.size(0))
        x_pooled, batch_pooled = self.reduce(x=x, so=so, batch=batch, return_batched=not self.sparse_output)
        edge_index_pooled, edge_weight_pooled = self.connect(edge_index=adj, so=so, edge_weight=edge_weight, batch=batch,
                                                             batch_pooled=batch_pooled)
        return PoolingOutput(x=x_pooled, edge_index=edge_index_pooled, edge_weight=edge_weight_pooled,
                             batch=batch_pooled, so=so)

    def precoarsening(self, edge_index=None, edge_weight: Optional[Tensor] = None, *, batch: Optional[Tensor] = None,
                      num_nodes: Optional[int] = None, **kwargs) -> PoolingOutput:
        """Precompute pooling outputs with a fixed assignment width ``k``."""
        return super().precoarsening(edge_index=edge_index, edge_weight=edge_weight, batch=batch, num_nodes=num_nodes,
                                     fixed_k=True, **kwargs)

    def extra_repr_args(self) -> dict:
        return {"batched": self.batched, "cached": self.cached}
