"""Auxiliary losses DiffPool / MinCut / DMoN / AsymCheegerCut / HOSC / BN-Pool compute between Reduce and Connect
(reference: tgp/utils/losses.py:39-123, 218-316, 392-483, 503-550, 597-708, 780-1010, 1083-1562).

The batched dense losses run on native kernels: the link-prediction residual is
reduced inside the GEMM epilogue so S S^T [B,N,N] is never materialised, the entropy and the
trace(S^T D S) terms are single-pass reductions, S^T S runs on the matrix cores; each has a closed-form
backward.  The unbatched (sparse-adjacency) variants are differentiable torch ops over the edge list.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import Tensor

from .. import eps
from .. import functions as Fn
from .. import kernels as K
from .ops import check_and_filter_edge_weights, graph_ptr, max_graph_size, num_graphs_of


def _reduce(loss: Tensor, how: str) -> Tensor:
    if how == "mean":
        return loss.mean(dim=0)
    if how == "sum":
        return loss.sum(dim=0)
    raise ValueError(f"Batch reduction {how} not allowed, must be one of ['mean', 'sum'].")


def _native_f32(*ts) -> bool:
    """float32 operands take the kernels (host tensors raise there: no CPU fallback); float64 takes the composed torch
    forms."""
    return not any(t is not None and t.dtype == torch.float64 for t in ts)


def _seg_sum(src: Tensor, index: Tensor, size: int) -> Tensor:
    return src.new_zeros((size,) + tuple(src.shape[1:])).index_add_(0, index, src)


class _CutDenFn(torch.autograd.Function):
    """den[b] = trace(S^T D S) = sum_i deg_i ||S_i||^2 with deg = row sums of adj, one pass over adj."""

    @staticmethod
    def forward(ctx, adj, S, graph_sizes=None):
        deg, q, den = K.cut_terms(adj, S, graph_sizes)
        ctx.save_for_backward(S, deg, q)
        return den

    @staticmethod
    def backward(ctx, g):
        S, deg, q = ctx.saved_tensors
        g = g.view(-1, 1, 1)
        g_adj = g_s = None
        if ctx.needs_input_grad[0]:
            g_adj = (g * q.unsqueeze(-1)).expand(-1, -1, q.size(1)).contiguous()
        if ctx.needs_input_grad[1]:
            g_s = 2.0 * g * deg.unsqueeze(-1) * S
        return g_adj, g_s, None


class _GramFn(torch.autograd.Function):
    """G = S^T S on the matrix cores (split over the node dimension); dS = S (g + g^T)."""

    @staticmethod
    def forward(ctx, S, graph_sizes=None):
        ctx.save_for_backward(S)
        return K.dense_pool(S, None, S, graph_sizes=graph_sizes)[0]

    @staticmethod
    def backward(ctx, g):
        (S,) = ctx.saved_tensors
        return K.bmm(S, (g + g.transpose(-1, -2)).contiguous()), None


class _LinkNormFn(torch.autograd.Function):
    """||adj - S S^T||_F over the whole batch; S S^T only ever exists tile by tile in the MFMA
    accumulators (forward) and the backward uses d/dS = (4 S S^T S - 2 (A + A^T) S) / (2 norm)."""

    @staticmethod
    def forward(ctx, S, adj, graph_sizes=None):
        norm = torch.sqrt(K.link_loss_sq(S, adj, graph_sizes).sum())
        ctx.save_for_backward(S, adj, norm)
        ctx.products = Fn.shared_products(S, adj)  # A S, A^T S: shared with DenseConnect's backward
        return norm

    @staticmethod
    def backward(ctx, g):
        S, adj, norm = ctx.saved_tensors
        coef = torch.where(norm > 0, g / norm, torch.zeros_like(norm))  # torch.norm's subgradient at 0
        g_s = g_adj = None
        if ctx.needs_input_grad[0]:
            gram = K.dense_pool(S, None, S)[0]
            g_s = (2.0 * K.bmm(S, gram) - ctx.products.get_u(S, adj) - ctx.products.get_v(S, adj)) * coef
        if ctx.needs_input_grad[1]:
            g_adj = (adj - torch.matmul(S, S.transpose(1, 2))) * coef
        return g_s, g_adj, None


class _EntropySumFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S):
        ctx.save_for_backward(S)
        return K.entropy_sum(S)

    @staticmethod
    def backward(ctx, g):
        (S,) = ctx.saved_tensors
        if S.is_cuda and S.dtype == torch.float32 and g.numel() == 1:
            return K.entropy_bwd(S, g)  # one elementwise launch
        return -(torch.log(S + eps) + S / (S + eps)) * g


def mincut_loss(adj: Tensor, S: Tensor, adj_pooled: Tensor, batch_reduction: str = "mean",
                graph_sizes: Optional[Tensor] = None) -> Tensor:
    """``graph_sizes`` (this build only): real nodes per graph of a zero-padded batch, lets the pass over adj skip the
    padding."""
    num = torch.diagonal(adj_pooled, dim1=-2, dim2=-1).sum(-1)
    den = _CutDenFn.apply(adj, S, graph_sizes)  # trace(S^T D S) without forming D
    return _reduce(-(num / (den + eps)), batch_reduction)


class _MinCutTermsFn(torch.autograd.Function):
    """[2,B] per-graph values of :func:`mincut_loss` and :func:`orthogonality_loss` under autograd with a native backward
    tail: forward = the three kernels of :func:`mincut_loss_terms`; backward = one launch for the K x K parts
    (tgp_mincut_loss_terms_bwd_f32), one product S (W + W^T) and one fused multiply-add for 2 c1 D S.  The adjacency gets
    no gradient here (callers whose adj requires one keep the composed Functions above)."""

    @staticmethod
    def forward(ctx, adj, S, raw, graph_sizes):
        deg, _, den = K.cut_terms(adj, S, graph_sizes)
        gram = K.dense_pool(S, None, S, graph_sizes=graph_sizes)[0]
        ctx.save_for_backward(S, raw, deg, den, gram)
        return K.mincut_loss_terms(raw, den, gram)

    @staticmethod
    def backward(ctx, g):
        S, raw, deg, den, gram = ctx.saved_tensors
        g_raw, c1, W = K.mincut_loss_terms_bwd(raw, den, gram, g)
        g_s = K.bmm(S, W + W.transpose(1, 2))
        g_s.addcmul_((2.0 * c1).view(-1, 1, 1) * deg.unsqueeze(-1), S)
        return None, g_s.to(S.dtype), g_raw.to(raw.dtype), None


def mincut_loss_terms(adj: Tensor, S: Tensor, adj_pooled: Tensor, graph_sizes: Optional[Tensor] = None) -> Tensor:
    """[2,B] per-graph values of :func:`mincut_loss` and :func:`orthogonality_loss` (before the batch reduction) for
    a device batch outside autograd: den and S^T S from their kernels, both tails in ONE launch."""
    _, _, den = K.cut_terms(adj, S, graph_sizes)
    gram = K.dense_pool(S, None, S, graph_sizes=graph_sizes)[0]
    return K.mincut_loss_terms(adj_pooled, den, gram)


class _OrthoFromGramFn(torch.autograd.Function):
    """l = || G / ||G||_F - I / sqrt(K) ||_F per graph (losses.py:59-70) with its closed-form gradient
    dl/dG = (Y - <Y, G> G / n^2) / (n l),  Y = G / n - I / sqrt(K),  n = ||G||_F."""

    @staticmethod
    def forward(ctx, gram):
        k = gram.size(-1)
        n = torch.linalg.matrix_norm(gram, keepdim=True)
        y = gram / n
        y.diagonal(dim1=-2, dim2=-1).sub_(1.0 / math.sqrt(k))
        l = torch.linalg.matrix_norm(y)
        ctx.save_for_backward(gram, n, y, l)
        return l

    @staticmethod
    def backward(ctx, g):
        gram, n, y, l = ctx.saved_tensors
        yg = (y * gram).sum(dim=(-2, -1), keepdim=True)
        coef = (g / l).view(-1, 1, 1) / n
        return coef * (y - yg * gram / (n * n))


def orthogonality_loss(S: Tensor, batch_reduction: str = "mean", graph_sizes: Optional[Tensor] = None) -> Tensor:
    if S.dim() == 2:  # a single graph [N,K]: the reference's transpose(-2,-1) / norm(dim=(-2,-1)) accept it (losses.py:59-70)
        return orthogonality_loss(S.unsqueeze(0), batch_reduction, None).reshape(())
    sts = _GramFn.apply(S, graph_sizes if S.dim() == 3 else None)
    if sts.is_cuda and torch.is_grad_enabled() and sts.requires_grad:
        return _reduce(_OrthoFromGramFn.apply(sts), batch_reduction)
    sts = sts / torch.norm(sts, dim=(-2, -1), keepdim=True)
    k = S.size(-1)
    target = torch.eye(k, device=S.device, dtype=S.dtype) / math.sqrt(k)
    return _reduce(torch.norm(sts - target, dim=(-2, -1)), batch_reduction)


def link_pred_loss(S: Tensor, adj: Tensor, normalize_loss: bool = True,
                   graph_sizes: Optional[Tensor] = None) -> Tensor:
    loss = _LinkNormFn.apply(S, adj, graph_sizes)
    return loss / adj.numel() if normalize_loss is True else loss


def unbatched_entropy_loss(S: Tensor, num_nodes: Optional[int] = None) -> Tensor:
    if num_nodes is None:
        num_nodes = S.size(0)
    if S.is_cuda and S.dtype == torch.float32 and S.numel() > 0:
        return _EntropySumFn.apply(S) / num_nodes  # the same sum as the batched form: one launch (+ one in backward)
    return (-(S * torch.log(S + eps)).sum(dim=-1)).sum() / num_nodes


def entropy_loss(S: Tensor, num_nodes: int) -> Tensor:
    return _EntropySumFn.apply(S) / num_nodes


def _edge_weights(edge_index: Tensor, edge_weight: Optional[Tensor], like: Tensor) -> Tensor:
    if edge_weight is None:
        return torch.ones(edge_index.size(1), device=like.device, dtype=like.dtype)
    return check_and_filter_edge_weights(edge_weight).view(-1).to(like.dtype)


def _batch_or_zeros(batch: Optional[Tensor], n: int, device) -> Tensor:
    return torch.zeros(n, dtype=torch.long, device=device) if batch is None else batch


def sparse_mincut_loss(edge_index: Tensor, S: Tensor, edge_weight: Optional[Tensor] = None,
                       batch: Optional[Tensor] = None, batch_reduction: str = "mean") -> Tensor:
    n = S.size(0)
    w = _edge_weights(edge_index, edge_weight, S)
    nb = num_graphs_of(batch)
    batch = _batch_or_zeros(batch, n, S.device)
    deg = _seg_sum(w, edge_index[0], n)
    den = _seg_sum(deg * (S * S).sum(-1), batch, nb)
    contrib = w * Fn.edge_dot(S, edge_index)
    num = _seg_sum(contrib, batch[edge_index[0]], nb)
    return _reduce(-(num / (den + eps)), batch_reduction)


def _per_graph_gram(S: Tensor, batch: Optional[Tensor], nb: int) -> Tensor:
    """[B,K,K] stack of S_g^T S_g (batch is sorted, as everywhere in PyG-style batching): one launch."""
    if batch is None or nb == 1:
        return Fn.bmm(S, S, trans_a=True).unsqueeze(0)
    _, ptr = graph_ptr(batch, nb)
    return Fn.segment_gemm_tn(S, S, ptr, max_graph_size(batch))


def unbatched_orthogonality_loss(S: Tensor, batch: Optional[Tensor] = None,
                                 batch_reduction: str = "mean") -> Tensor:
    n, k = S.shape
    nb = num_graphs_of(batch)
    gram = _per_graph_gram(S, batch, nb)
    gram = gram / torch.norm(gram, dim=(-2, -1), keepdim=True)
    target = torch.eye(k, device=S.device, dtype=S.dtype) / math.sqrt(k)
    return _reduce(torch.norm(gram - target, dim=(-2, -1)), batch_reduction)


def sparse_link_pred_loss(S: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None,
                          batch: Optional[Tensor] = None, normalize_loss: bool = True) -> Tensor:
    n = S.size(0)
    w = _edge_weights(edge_index, edge_weight, S)
    nb = num_graphs_of(batch)
    ss = Fn.edge_dot(S, edge_index)
    gram = _per_graph_gram(S, batch, nb)
    # ||A - S S^T||_F^2 = sum_E (w - ss)^2 + sum_g ||S_g^T S_g||_F^2 - sum_E ss^2
    sq = ((w - ss) ** 2).sum() + (gram * gram).sum() - (ss ** 2).sum()
    loss = torch.sqrt(torch.clamp(sq, min=0.0))
    if not normalize_loss:
        return loss
    if batch is None:
        return loss / (n * n) if n > 0 else loss
    sizes, _ = graph_ptr(batch, nb)
    return loss / (sizes * sizes).sum().clamp(min=1)  # stays on the device: no host round trip


# ------------------------------------------------------------------------------------------------ DMoN
class _DMoNTermsFn(torch.autograd.Function):
    """[3,B] per-graph spectral, cluster and orthogonality terms of DMoN (utils/losses.py:1083-1265 and :59-70) with a
    native backward.  Forward: the partial pass over S (behind one pass over adj for the degrees, ``layout`` "dense"),
    S^T S when ``want_ortho``, one tail launch.  Backward: one launch for the per-graph coefficients and W, the product
    S (W + W^T), one elementwise pass for dS = alpha_b d ca_b + beta_b cs_b; the gradient of raw is -(g_spec / 2m) I,
    that of ``tr`` -g_spec / 2m.  Neither the adjacency nor the degrees get a gradient here.

    ``layout``: ("dense", mask, graph_sizes[, deg [B,N]]) with ``source`` = adj [B,N,N] or None (then the degrees given,
    or none), or ("flat", ptr, batch, max_nodes) with ``source`` = deg [Ntot] or None.  ``coeffs``: the three rows come out times these (the pooler's loss
    coefficients: no separate scaling launch)."""

    @staticmethod
    def forward(ctx, S, raw, tr, source, layout, want_ortho, sqrt_k, clamp_m, coeffs):
        if layout[0] == "dense":
            deg, part = K.dmon_dense_terms(source, S, layout[1], layout[2], deg=layout[3] if len(layout) > 3 else None)
            gram = K.dense_pool(S, None, S, graph_sizes=layout[2])[0] if want_ortho else None
        else:
            deg = source
            part = K.dmon_node_terms(S, deg, layout[1], layout[3])
            gram = None
        out, ca, cs, stats = K.dmon_loss_terms(part, raw, tr, gram, sqrt_k, clamp_m, coeffs)
        ctx.save_for_backward(S, deg, ca, cs, stats, gram)
        ctx.layout, ctx.sqrt_k, ctx.coeffs = layout, sqrt_k, coeffs
        ctx.has_raw, ctx.has_tr = raw is not None, tr is not None
        return out

    @staticmethod
    def backward(ctx, g):
        S, deg, ca, cs, stats, gram = ctx.saved_tensors
        g_raw, g_tr, coef, W = K.dmon_loss_terms_bwd(g, stats, gram, S.size(-1), ctx.sqrt_k,
                                                     ctx.has_raw and ctx.needs_input_grad[1],
                                                     ctx.has_tr and ctx.needs_input_grad[2], ctx.coeffs)
        g_s = None
        if ctx.needs_input_grad[0]:
            acc = W is not None
            g_s = K.bmm(S, W + W.transpose(1, 2)) if acc else torch.empty(S.shape, dtype=torch.float32, device=S.device)
            if ctx.layout[0] == "dense":
                K.dmon_ds(deg, ca, cs, coef, S.size(0) * S.size(1), S.size(1), None, g_s, acc)
            else:
                K.dmon_ds(deg, ca, cs, coef, S.size(0), max(S.size(0), 1), ctx.layout[2], g_s, acc)
            g_s = g_s.to(S.dtype)
        return g_s, g_raw, g_tr, None, None, None, None, None, None


_ONES3 = (1.0, 1.0, 1.0)


def dmon_loss_terms(adj: Optional[Tensor], S: Tensor, adj_pooled: Tensor, mask: Optional[Tensor] = None,
                    graph_sizes: Optional[Tensor] = None, coeffs=(1.0, 1.0, 1.0), deg: Optional[Tensor] = None) -> Tensor:
    """[3,B]: per-graph values of :func:`spectral_loss`, :func:`cluster_loss` and :func:`orthogonality_loss` (before the
    batch reduction) of a padded batch, each times its coefficient in ``coeffs``, float32 device operands: one pass over
    adj (or ``adj`` None and the degrees ``deg`` [B,N] given), one over S, S^T S, one tail launch.  ``graph_sizes`` (this
    build only): real nodes per graph of a zero-padded batch, lets the passes skip the padding."""
    return _DMoNTermsFn.apply(S, adj_pooled, None, adj, ("dense", mask, graph_sizes, deg), True,
                              math.sqrt(S.size(-1)), False, tuple(float(c) for c in coeffs))


def spectral_loss(adj: Tensor, S: Tensor, adj_pooled: Tensor, mask: Optional[Tensor] = None,
                  num_supernodes: Optional[int] = None, batch_reduction: str = "mean") -> Tensor:
    """DMoN's spectral (modularity) loss -(trace(S^T A S) - ||S^T d||^2 / 2m) / 2m per graph, d the (masked) row sums of
    ``adj``, 0 for a graph without edges (reference utils/losses.py:1083-1148)."""
    if _native_f32(adj, S, adj_pooled) and S.dim() == 3 and not adj.requires_grad:
        terms = _DMoNTermsFn.apply(S, adj_pooled, None, adj, ("dense", mask, None), False, 1.0, False, _ONES3)
        return _reduce(terms[0], batch_reduction)
    if mask is None:
        mask = torch.ones(S.size(0), S.size(1), dtype=torch.bool, device=S.device)
    deg = adj.sum(-1) * mask
    m = deg.sum(-1) / 2
    safe_m = torch.where(m > 0, m, torch.ones_like(m))
    ca = torch.einsum("bnk,bn->bk", S, deg)
    tr = torch.diagonal(adj_pooled, dim1=-2, dim2=-1).sum(-1)
    loss = -(tr - (ca * ca).sum(-1) / (2 * safe_m)) / (2 * safe_m)
    return _reduce(torch.where(m > 0, loss, torch.zeros_like(loss)), batch_reduction)


def cluster_loss(S: Tensor, mask: Optional[Tensor] = None, num_supernodes: Optional[int] = None,
                 batch_reduction: str = "mean") -> Tensor:
    """DMoN's cluster loss ||S^T 1|| sqrt(K) / n - 1 per graph, n = mask.sum(1) (N without a mask)
    (reference utils/losses.py:1216-1265)."""
    k = S.size(-1) if num_supernodes is None else num_supernodes
    if _native_f32(S) and S.dim() == 3:
        terms = _DMoNTermsFn.apply(S, None, None, None, ("dense", mask, None), False, math.sqrt(k), False, _ONES3)
        return _reduce(terms[1], batch_reduction)
    n = S.size(1) if mask is None else mask.sum(dim=1)
    return _reduce(torch.norm(S.sum(1), dim=1) / n * math.sqrt(k) - 1, batch_reduction)


def _flat_layout(S: Tensor, batch: Optional[Tensor]):
    """("flat", ptr, batch, max_nodes) of a sorted batch vector, or None when the batch is not sorted."""
    n = S.size(0)
    if batch is None:
        return ("flat", Fn._whole_range(n, S.device), None, n)
    from .ops import batch_info
    info = batch_info(batch)
    if not info.is_sorted:
        return None
    return ("flat", info.ptr, batch, info.max_nodes)


def sparse_spectral_loss(edge_index: Tensor, S: Tensor, edge_weight: Optional[Tensor] = None,
                         batch: Optional[Tensor] = None, batch_reduction: str = "mean") -> Tensor:
    """The spectral loss of an edge list (reference utils/losses.py:1151-1213): out-degrees scatter(w, edge_index[0]),
    trace(S_g^T A_g S_g) = sum over the graph's edges of w (S_src . S_dst), m_g clamped to eps."""
    n = S.size(0)
    w = _edge_weights(edge_index, edge_weight, S)
    nb = num_graphs_of(batch)
    bvec = _batch_or_zeros(batch, n, S.device)
    src = edge_index[0]
    deg = _seg_sum(w, src, n)
    layout = _flat_layout(S, batch) if _native_f32(S, w) and S.dim() == 2 and n > 0 else None
    if layout is not None and not w.requires_grad:
        tr = _seg_sum(w * Fn.edge_dot(S, edge_index), bvec[src], nb)
        return _reduce(_DMoNTermsFn.apply(S, None, tr, deg, layout, False, 1.0, True, _ONES3)[0], batch_reduction)
    tr = _seg_sum(w * (S[src] * S[edge_index[1]]).sum(-1), bvec[src], nb)
    m = (_seg_sum(w, bvec[src], nb) / 2).clamp(min=eps)
    ca = _seg_sum(S * deg.unsqueeze(-1), bvec, nb)
    return _reduce(-(tr - (ca * ca).sum(-1) / (2 * m)) / (2 * m), batch_reduction)


def unbatched_cluster_loss(S: Tensor, batch: Optional[Tensor] = None, batch_reduction: str = "mean") -> Tensor:
    """The cluster loss of an un-padded batch (reference utils/losses.py:435-473): ||S_g^T 1|| sqrt(K) / n_g - 1."""
    n, k = S.shape
    layout = _flat_layout(S, batch) if _native_f32(S) and n > 0 else None
    if layout is not None:
        terms = _DMoNTermsFn.apply(S, None, None, None, layout, False, math.sqrt(k), True, _ONES3)
        return _reduce(terms[1], batch_reduction)
    nb = num_graphs_of(batch)
    bvec = _batch_or_zeros(batch, n, S.device)
    sizes = torch.bincount(bvec, minlength=nb)[:nb].to(S.dtype)
    return _reduce(torch.norm(_seg_sum(S, bvec, nb), dim=1) / sizes * math.sqrt(k) - 1, batch_reduction)


# ------------------------------------------------------------------------------------------------ Just Balance
class _JBTermsFn(torch.autograd.Function):
    """[B] per-graph values of Just Balance's loss -sum_k sqrt(sum_i S_ik^2 + eps) / sqrt(n_b K), times ``scale``
    (utils/losses.py:553-594, 1013-1080), with a native backward.  Forward: one launch when no graph has more than 64
    rows, else the partial pass over S and a tail; the tail leaves coef [B,K].  Backward: one elementwise launch
    dS = g_b coef_bk S.

    ``layout``: ("dense", mask, graph_sizes, num_nodes) for S [B,N,K] or ("flat", ptr, batch, max_nodes) for S [Ntot,K]
    of a sorted batch."""

    @staticmethod
    def forward(ctx, S, layout, normalize, num_supernodes, scale):
        if layout[0] == "dense":
            out, coef = K.jb_terms(S, mask=layout[1], graph_sizes=layout[2], normalize=normalize, num_nodes=layout[3],
                                   num_supernodes=num_supernodes, scale=scale)
        else:
            out, coef = K.jb_terms(S, ptr=layout[1], max_nodes=layout[3], normalize=normalize,
                                   num_supernodes=num_supernodes, scale=scale)
        ctx.save_for_backward(S, coef)
        ctx.batch = None if layout[0] == "dense" else layout[2]
        return out

    @staticmethod
    def backward(ctx, g):
        S, coef = ctx.saved_tensors
        g_s = K.jb_ds(S, coef, g, ctx.batch).to(S.dtype) if ctx.needs_input_grad[0] else None
        return g_s, None, None, None, None


def _jb_native(S: Tensor, batch: Optional[Tensor] = None) -> bool:
    """The kernels take a float32 device S (un-padded: of a sorted batch); float64, host tensors and an unsorted batch
    vector take the composed torch form."""
    if not (S.is_cuda and S.dtype == torch.float32 and S.numel() > 0):
        return False
    if S.dim() == 3 or batch is None:
        return True
    from .ops import batch_info
    return batch_info(batch).is_sorted  # (memoised per batch vector)


def jb_loss_terms(S: Tensor, mask: Optional[Tensor] = None, graph_sizes: Optional[Tensor] = None,
                  batch: Optional[Tensor] = None, normalize_loss: bool = True, num_nodes: Optional[int] = None,
                  num_supernodes: Optional[int] = None, scale: float = 1.0) -> Tensor:
    """[B]: per-graph values of :func:`just_balance_loss` (S [B,N,K], ``mask``; ``graph_sizes``, this build only: real
    nodes per graph of a batch whose padded rows of S are zero, lets the pass skip them) or of
    :func:`unbatched_just_balance_loss` (S [Ntot,K], ``batch``), before the batch reduction, times ``scale``.  Only the
    diagonal of S^T S is computed.  float32 device S (and a sorted batch): the kernels; otherwise torch ops."""
    k = S.size(-1) if num_supernodes is None else num_supernodes
    if S.dim() == 3:
        if _jb_native(S):
            return _JBTermsFn.apply(S, ("dense", mask, graph_sizes, num_nodes), bool(normalize_loss), k, float(scale))
        loss = -torch.sqrt((S * S).sum(dim=1) + eps).sum(dim=-1)
        if normalize_loss:
            if mask is None:
                n = S.size(1) if num_nodes is None else num_nodes
                loss = loss / torch.tensor(n * k, dtype=loss.dtype, device=loss.device).sqrt()
            else:
                loss = loss / (mask.sum(dim=1).to(loss.dtype) * float(k)).sqrt()
        return loss if scale == 1 else loss * scale
    n = S.size(0)
    if _jb_native(S, batch):
        return _JBTermsFn.apply(S, _flat_layout(S, batch), bool(normalize_loss), S.size(1), float(scale))
    bvec = _batch_or_zeros(batch, n, S.device)
    nb = num_graphs_of(batch)
    loss = -torch.sqrt(_seg_sum(S * S, bvec, nb) + eps).sum(dim=-1)
    if normalize_loss:
        sizes = torch.bincount(bvec, minlength=nb)[:nb].to(loss.dtype)
        loss = loss / (sizes * float(S.size(1))).sqrt()
    return loss if scale == 1 else loss * scale


def jb_loss_mean(S: Tensor, mask: Optional[Tensor] = None, graph_sizes: Optional[Tensor] = None,
                 batch: Optional[Tensor] = None, normalize_loss: bool = True, num_nodes: Optional[int] = None,
                 num_supernodes: Optional[int] = None, scale: float = 1.0) -> Tensor:
    """The batch mean of :func:`jb_loss_terms` (what the pooler hands out).  Inference on the kernels' path is ONE native
    call: no autograd node, no coefficients for a backward, the mean from a launch of the same call; with
    ``graph_sizes`` they also give n_b, which the mask would only count again."""
    if _jb_native(S, batch) and not (torch.is_grad_enabled() and S.requires_grad):
        k = S.size(-1) if num_supernodes is None else num_supernodes
        if S.dim() == 3:
            return K.jb_terms(S, mask=None if graph_sizes is not None else mask, graph_sizes=graph_sizes,
                              normalize=bool(normalize_loss), num_nodes=num_nodes, num_supernodes=k, scale=float(scale),
                              want_coef=False, want_mean=True)[2]
        layout = _flat_layout(S, batch)
        return K.jb_terms(S, ptr=layout[1], max_nodes=layout[3], normalize=bool(normalize_loss), scale=float(scale),
                          want_coef=False, want_mean=True)[2]
    return jb_loss_terms(S, mask, graph_sizes, batch, normalize_loss, num_nodes, num_supernodes, scale).mean()


def just_balance_loss(S: Tensor, mask: Optional[Tensor] = None, normalize_loss: bool = True,
                      num_nodes: Optional[int] = None, num_supernodes: Optional[int] = None,
                      batch_reduction: str = "mean") -> Tensor:
    """Just Balance's loss -trace(sqrt(S^T S + eps)) per graph of a padded batch S [B,N,K], over ALL N rows of S (the
    mask only counts n_b); ``normalize_loss``: divided by sqrt(n_b K), n_b = mask.sum(1), without a mask ``num_nodes``
    (default N); K = ``num_supernodes`` (default the columns of S) (reference utils/losses.py:1013-1080)."""
    return _reduce(jb_loss_terms(S, mask, None, None, normalize_loss, num_nodes, num_supernodes), batch_reduction)


def unbatched_just_balance_loss(S: Tensor, batch: Optional[Tensor] = None, normalize_loss: bool = True,
                                batch_reduction: str = "mean") -> Tensor:
    """The same loss of an un-padded batch S [Ntot,K]: graph g owns the rows with batch == g (None: one graph),
    n_g = their number (reference utils/losses.py:553-594)."""
    return _reduce(jb_loss_terms(S, batch=batch, normalize_loss=normalize_loss), batch_reduction)


# ------------------------------------------------------------------------------------------------ AsymCheegerCut
class _ACCTermsFn(torch.autograd.Function):
    """[2,B] per-graph total-variation and balance (asymmetric norm) terms of AsymCheegerCut pooling
    (utils/losses.py:503-550, 780-1010), each times its coefficient in ``coeffs``, with a native backward.

    Forward: the pass over the nonzeros of the adjacency (``layout`` "dense") or over every node's out-edges ("flat"),
    the quantile select with the asymmetric-norm column sums, one tail launch.  Backward: dS of the total variation
    (row i and column i of the adjacency; out- and in-edges of node i), then one elementwise pass that adds dS of the
    balance term.  Neither the adjacency nor the edge weights get a gradient here.

    ``layout``: ("dense", mask, graph_sizes) with ``source`` = adj [B,N,N] or None (no total variation), or
    ("flat", ptr, batch, max_nodes) with ``source`` = (edge_index, edge_weight or None) or None.  ``k`` <= 1: no
    balance term (0).  Ties: where several nodes of a graph hold a column's quantile value, the LOWEST node index
    receives the quantile's gradient (the reference's unstable sort leaves that open)."""

    @staticmethod
    def forward(ctx, S, source, layout, k, coeffs):
        dense = layout[0] == "dense"
        dev = K.N.require_device(S)
        tv = groups = sel = None
        if dense:
            B, Kc = S.size(0), S.size(2)
            if source is not None:
                tv = ("dense",) + K.acc_tv_dense(source, S, layout[2])
            if k > 1:
                sel = K.acc_quantile(S, k, mask=layout[1], graph_sizes=layout[2])
        else:
            B, Kc = layout[1].numel() - 1, S.size(1)
            if source is not None:
                groups = K.edge_group(source[0], S.size(0))  # (by source; by destination: in the backward)
                tv = ("edge", K.acc_tv_edge(S, source[0], source[1], groups), groups, layout[1])
            if k > 1:
                sel = K.acc_quantile(S, k, ptr=layout[1], max_nodes=layout[3])
        out, ecnt = K.acc_tail(B, Kc, k, dev, tv, None if sel is None else sel[2], None if sel is None else sel[4],
                                     coeffs)
        ctx.save_for_backward(S, ecnt, *(sel[:2] + sel[3:5] if sel is not None else ()))
        ctx.source, ctx.layout, ctx.k, ctx.coeffs, ctx.groups = source, layout, k, coeffs, groups
        return out

    @staticmethod
    def backward(ctx, g):
        S, ecnt, *sel = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        g = g.to(torch.float32).contiguous()
        layout, source, dense = ctx.layout, ctx.source, ctx.layout[0] == "dense"
        ds = None
        if source is not None and dense:
            ds = K.acc_tv_dense_bwd(source, S, layout[2], g[0], ecnt, ctx.coeffs[0])
        elif source is not None:
            by_dst = K.edge_group(source[0], S.size(0), by_destination=True)
            ds = K.acc_tv_edge_bwd(S, source[0], source[1], ctx.groups, by_dst, layout[2], g[0], ecnt, ctx.coeffs[0])
        if sel:
            acc = ds is not None
            if not acc:
                ds = torch.empty(S.shape, dtype=torch.float32, device=S.device)
            q, qnode, cge, nreal = sel
            if dense:
                K.acc_asym_bwd(S, ctx.k, q, qnode, cge, nreal, g[1], ctx.coeffs[1], ds, acc, mask=layout[1],
                               graph_sizes=layout[2])
            else:
                K.acc_asym_bwd(S, ctx.k, q, qnode, cge, nreal, g[1], ctx.coeffs[1], ds, acc, ptr=layout[1],
                               batch=layout[2])
        if ds is None:
            ds = torch.zeros(S.shape, dtype=torch.float32, device=S.device)
        return ds.view(S.shape).to(S.dtype), None, None, None, None


_ONES2 = (1.0, 1.0)


def acc_loss_terms(adj: Optional[Tensor], S: Tensor, k: int, mask: Optional[Tensor] = None,
                   graph_sizes: Optional[Tensor] = None, coeffs=(1.0, 1.0)) -> Tensor:
    """[2,B]: per-graph values of :func:`totvar_loss` and :func:`asym_norm_loss` (before the batch reduction) of a padded
    batch, each times its coefficient in ``coeffs``; float32 device operands.  ``graph_sizes`` (this build only): real
    nodes per graph of a zero-padded batch, lets the passes skip the padding."""
    return _ACCTermsFn.apply(S, adj, ("dense", mask, graph_sizes), int(k), tuple(float(c) for c in coeffs))


def acc_sparse_loss_terms(edge_index: Tensor, edge_weight: Optional[Tensor], S: Tensor, k: int,
                          batch: Optional[Tensor] = None, coeffs=(1.0, 1.0)) -> Optional[Tensor]:
    """[2,B]: per-graph values of :func:`sparse_totvar_loss` and :func:`unbatched_asym_norm_loss` of an un-padded batch,
    each times its coefficient, from ONE Function (one tail launch); None when the operands take the composed forms
    (float64, edge weights that require grad, an unsorted batch, no nodes)."""
    w = None if edge_weight is None else check_and_filter_edge_weights(edge_weight).view(-1)
    if not (_native_f32(S, w) and S.dim() == 2 and S.size(0) > 0) or (w is not None and w.requires_grad):
        return None
    K.N.require_device(S, edge_index, w, batch)
    layout = _flat_layout(S, batch)
    if layout is None:
        return None
    return _ACCTermsFn.apply(S, (edge_index, w), layout, int(k), tuple(float(c) for c in coeffs))


def totvar_loss(S: Tensor, adj: Tensor, batch_reduction: str = "mean") -> Tensor:
    """The total-variation loss sum_ij a_ij ||s_i - s_j||_1 / (2 E) per graph, E = the nonzero entries of ``adj[b]``
    clamped to >= 1 (reference utils/losses.py:780-862).  Padded rows are zero and add nothing; no mask is read."""
    if _native_f32(S, adj) and S.dim() == 3 and not adj.requires_grad:
        return _reduce(_ACCTermsFn.apply(S, adj, ("dense", None, None), 0, _ONES2)[0], batch_reduction)
    b, i, j = adj.nonzero(as_tuple=True)  # (row-major: a fixed summation order)
    dist = (S[b, i] - S[b, j]).abs().sum(-1)
    tv = _seg_sum(adj[b, i, j] * dist, b, S.size(0))
    edges = torch.bincount(b, minlength=S.size(0)).clamp(min=1)
    return _reduce(tv / (2 * edges), batch_reduction)


def sparse_totvar_loss(edge_index: Tensor, S: Tensor, edge_weight: Optional[Tensor] = None,
                       batch: Optional[Tensor] = None, batch_reduction: str = "mean") -> Tensor:
    """The total-variation loss of an edge list (reference utils/losses.py:865-917): E counts every edge whose source
    lies in the graph, zero-weight ones included (the dense form counts nonzero entries)."""
    n = S.size(0)
    w = None if edge_weight is None else check_and_filter_edge_weights(edge_weight).view(-1)
    if _native_f32(S, w) and S.dim() == 2 and not (w is not None and w.requires_grad):
        K.N.require_device(S, edge_index, w, batch)
        layout = _flat_layout(S, batch) if n > 0 else None
        if layout is not None:
            return _reduce(_ACCTermsFn.apply(S, (edge_index, w), layout, 0, _ONES2)[0], batch_reduction)
    nb = num_graphs_of(batch)
    src, dst = edge_index[0], edge_index[1]
    graph = _batch_or_zeros(batch, n, S.device)[src]
    dist = (S[src] - S[dst]).abs().sum(-1)
    tv = _seg_sum(dist if w is None else w.to(S.dtype) * dist, graph, nb)
    edges = torch.bincount(graph, minlength=nb)[:nb].clamp(min=1)
    return _reduce(tv / (2 * edges), batch_reduction)


def _asym_norm_composed(S: Tensor, k: int, graph: Tensor, nb: int) -> Tensor:
    """[nb] balance terms of the rows of S [Ntot,K] grouped by ``graph``, as torch ops (any dtype, any row order)."""
    out = []
    for b in range(nb):
        rows = S[graph == b]
        n = rows.size(0)
        beta = n * (k - 1)
        if beta == 0:
            out.append(S.new_zeros(()))
            continue
        q = rows.sort(dim=0, descending=True)[0][min(n // k, n - 1)]
        d = rows - q
        out.append((beta - torch.where(d >= 0, (k - 1) * d, -d).sum()) / beta)
    return torch.stack(out) if out else S.new_zeros(0)


def asym_norm_loss(S: Tensor, k: int, mask: Optional[Tensor] = None, batch_reduction: str = "mean") -> Tensor:
    """The asymmetric-norm (balance) loss (n (k-1) - sum_ik rho(s_ik - q_k)) / (n (k-1)) per graph: q_k the entry at position
    min(floor(n / k), n - 1) of column k sorted in descending order, n the graph's real nodes (``mask``; N without one),
    rho(d) = (k-1) d for d >= 0 and -d below; 0 when k <= 1 or n (k-1) == 0 (reference utils/losses.py:920-1010).

    The quantile is differentiable: its gradient lands on the node that supplied it, and where several nodes tie at the
    quantile value, on the LOWEST node index among them (the reference's unstable sort leaves that open)."""
    B, n = S.size(0), S.size(1)
    if k <= 1 or n == 0:
        return _reduce(S.new_zeros(B), batch_reduction)
    if _native_f32(S) and S.dim() == 3:
        return _reduce(_ACCTermsFn.apply(S, None, ("dense", mask, None), int(k), _ONES2)[1], batch_reduction)
    if mask is None:
        mask = torch.ones(B, n, dtype=torch.bool, device=S.device)
    graph = torch.arange(B, device=S.device).unsqueeze(1).expand(B, n)[mask]
    # (every graph of the batch has a term, 0 for one without real nodes, as the kernels have it; the reference drops
    #  trailing graphs whose mask is empty from the mean)
    return _reduce(_asym_norm_composed(S[mask], k, graph, B), batch_reduction)


def unbatched_asym_norm_loss(S: Tensor, k: int, batch: Optional[Tensor] = None, batch_reduction: str = "mean") -> Tensor:
    """The balance loss of an un-padded batch (reference utils/losses.py:503-550); ties as :func:`asym_norm_loss`."""
    n = S.size(0)
    if k <= 1:
        return S.new_zeros(())
    if _native_f32(S) and S.dim() == 2:
        K.N.require_device(S, batch)
        layout = _flat_layout(S, batch) if n > 0 else None
        if layout is not None:
            return _reduce(_ACCTermsFn.apply(S, None, layout, int(k), _ONES2)[1], batch_reduction)
    graph = _batch_or_zeros(batch, n, S.device)
    return _reduce(_asym_norm_composed(S, k, graph, int(graph.max()) + 1 if n else 0), batch_reduction)


# ------------------------------------------------------------------------------------------------ HOSC
def _hosc_csr(edge_index: Tensor, w: Optional[Tensor], n: int):
    """(edge_index, weights or None, int32 row offsets) of the row-sorted, duplicate-summed list: the CSR form of the A
    the reference's ``sparse_coo_tensor(...).coalesce()`` builds (rows = sources)."""
    ones = w is None
    if ones and K.coalesced_memo(edge_index, n):
        ei, w2 = edge_index, None
    else:
        ei, w2 = Fn.coalesce_sum(edge_index, torch.ones(edge_index.size(1), device=edge_index.device) if ones
                                 else w.detach(), n)
    if ones and ei is edge_index:
        w2 = None  # (nothing merged: the weights are still all one)
    return ei, w2, K.csr_offsets(ei, n)


def _hosc_chain_csr(csr, S: Tensor, n: int, rounds: int):
    """[T1, ..] with T1 = A [S | 1], T2 = A T1, T3 = A T2 for the first ``rounds`` of them: Z and the degree vector ride
    together, K + 1 columns padded with zeros to a multiple of four (rows of 16-byte vectors for the CSR product)."""
    ei, w, row_ptr = csr
    kc = S.size(1)
    t = torch.nn.functional.pad(S.detach().to(torch.float32), (0, -(-(kc + 1) // 4) * 4 - kc))
    t[:, kc] = 1.0
    out = []
    for _ in range(rounds):
        t = K.spmm_csr(row_ptr, ei, w, n, t)
        out.append(t)
    return out


class _HOSCTermsFn(torch.autograd.Function):
    """[2,B] per-graph terms of HOSC pooling (reference poolers/hosc.py:269-376, utils/losses.py:218-316, 392-432,
    597-641): row 0 = ((1 - alpha) cut + alpha ho_cut) / k, row 1 = mu x orthogonality, with a native backward.  The motif
    adjacency A A A is never formed: ho_cut = -sum S (.) A (A (A S)) / (sum_i d_i |S_i|^2 + eps), d = A (A (A 1)).

    Forward, ``layout`` ("dense", mask, graph_sizes) with ``source`` = adj [B,N,N] or None (orthogonality only): three
    matrix-vector passes over adj, three products on the matrix cores, one pass over S / Z / d, S^T S for MinCut's
    orthogonality, one tail launch -- or, for N, K <= 64, ONE launch in front of the tail.  ``layout`` ("flat", ptr, batch,
    max_nodes) with ``source`` = (edge_index, weights or None, row offsets) of the coalesced list: three CSR products on
    [S | 1], the pass, the tail.  With alpha = 0 the chain is not run, with alpha = 1 the first-order cut is not evaluated.

    Backward: one launch for the per-graph coefficients (and W, g_raw), Zt = A^T (A^T (A^T S)) -- skipped when the
    adjacency is known to be symmetric -- and one elementwise launch for dS.  The adjacency gets no gradient here.
    ``cfg`` = (alpha, mu, 1 / k, hosc_ortho).  ``raw`` [B,K,K] (dense layout) supplies trace(S^T A S) of the first-order
    cut; without it, the first product A S does."""

    @staticmethod
    def forward(ctx, S, raw, source, layout, cfg):
        alpha, mu, inv_k, hosc_ortho = cfg
        dense = layout[0] == "dense"
        kc = S.size(-1)
        want_cut = source is not None and alpha < 1
        want_ho = source is not None and alpha > 0
        z = z1 = d1 = d3 = gram = sym = None
        needs_grad = ctx.needs_input_grad[0]
        if dense:
            mask, sizes = layout[1], layout[2]
            n = S.size(1)
            if want_ho and K.hosc_is_small(n, kc):
                z, d1, d3, part = K.hosc_small(source, S, mask, sizes)
                if want_cut and raw is None:
                    z1 = K.bmm(source, S)
                    part = K.hosc_node_terms(S, z, z1, d3, d1, mask, sizes)
            else:
                if want_cut or want_ho:
                    d1 = K.hosc_matvec(source, None, sizes)
                if want_cut and raw is None:
                    z1 = K.bmm(source, S)
                if want_ho:
                    d3 = K.hosc_matvec(source, K.hosc_matvec(source, d1, sizes), sizes)
                    z = K.bmm(source, K.bmm(source, z1 if z1 is not None else K.bmm(source, S)))
                part = K.hosc_node_terms(S, z, z1, d3, d1 if want_cut else None, mask, sizes)
            if not want_cut:
                d1 = None
            if mu != 0 and not hosc_ortho:
                gram = K.dense_pool(S, None, S, graph_sizes=sizes)[0]
            if needs_grad and want_ho and source.dtype == torch.float32 and source.is_contiguous():
                sym = K.AdjSymmetry.of_dense(source)
        else:
            n = S.size(0)
            if want_cut or want_ho:
                ts = _hosc_chain_csr(source, S, n, 3 if want_ho else 1)
                if want_cut:
                    z1, d1 = ts[0][:, :kc], ts[0][:, kc]
                if want_ho:
                    z, d3 = ts[2][:, :kc], ts[2][:, kc]
                if needs_grad:
                    sym = K.AdjSymmetry.of_edge_list(source[0], source[1], source[0], source[1], source[2], n)
            part = K.hosc_node_terms(S, z, z1, d3, d1, ptr=layout[1], max_nodes=layout[3])
        out, cn, stats = K.hosc_loss_terms(part, kc, raw if want_cut else None, gram, alpha, mu, inv_k, hosc_ortho)
        adj = source if dense and (z is not None or z1 is not None) else None  # (the backward's A^T products read it)
        ctx.save_for_backward(S, stats, cn if (hosc_ortho and mu != 0 and kc > 1) else None, gram, z, z1, d3, d1, adj)
        ctx.layout, ctx.cfg, ctx.sym = layout, cfg, sym
        ctx.csr = source if not dense else None
        ctx.has_raw = raw is not None and want_cut
        return out

    @staticmethod
    def backward(ctx, g):
        S, stats, cn, gram, z, z1, d3, d1, adj = ctx.saved_tensors
        alpha, mu, inv_k, hosc_ortho = ctx.cfg
        kc = S.size(-1)
        g_raw, coef, W = K.hosc_loss_terms_bwd(g, stats, gram, kc, alpha, mu, inv_k, hosc_ortho,
                                               ctx.has_raw and ctx.needs_input_grad[1])
        g_s = None
        if ctx.needs_input_grad[0]:
            acc = W is not None
            g_s = K.bmm(S, W + W.transpose(1, 2)) if acc else torch.empty(S.shape, dtype=torch.float32, device=S.device)
            zt = z1t = None
            if (z is not None or z1 is not None) and not (ctx.sym is not None and ctx.sym.get()):
                if ctx.layout[0] == "dense":
                    u = K.bmm(adj, S, trans_a=True)
                    z1t = u if z1 is not None else None
                    if z is not None:
                        zt = K.bmm(adj, K.bmm(adj, u, trans_a=True), trans_a=True)
                else:  # the by-destination CSR (A^T), built here only
                    ei, w, _ = ctx.csr
                    n = S.size(0)
                    csr_t = _hosc_csr(ei.flip(0), w, n)
                    u = S.detach().to(torch.float32)
                    ts = []
                    for _ in range(3 if z is not None else 1):
                        u = K.spmm_csr(csr_t[2], csr_t[0], csr_t[1], n, u)
                        ts.append(u)
                    z1t = ts[0] if z1 is not None else None
                    zt = ts[2] if z is not None else None
            if ctx.layout[0] == "dense":
                K.hosc_ds(S, z, zt, z1, z1t, d3, d1, cn, coef, S.size(1), None, g_s, acc)
            else:
                K.hosc_ds(S, z, zt, z1, z1t, d3, d1, cn, coef, max(S.size(0), 1), ctx.layout[2], g_s, acc)
            g_s = g_s.view(S.shape).to(S.dtype)
        return g_s, g_raw, None, None, None


def _hosc_cfg(alpha, mu, k, hosc_ortho):
    return (float(alpha), float(mu), 1.0 / k, bool(hosc_ortho))


def _hosc_ortho_composed(S: Tensor, n) -> Tensor:
    """(sqrt(K) - sum_j ||S_*j|| / sqrt(n)) / (sqrt(K) - 1) per graph of S [B,N,K] as torch ops; n: a number or the
    integer tensor mask.sum(1), whose square root the reference takes in float32 whatever S's dtype (losses.py:638)."""
    sqrt_k = math.sqrt(S.size(-1))
    sqrt_n = n.sqrt() if isinstance(n, Tensor) else math.sqrt(n)
    return (sqrt_k - torch.norm(S, dim=-2).sum(-1) / sqrt_n) / (sqrt_k - 1)


def _ho_cut_composed_dense(adj: Tensor, S: Tensor) -> Tensor:
    """-sum S (.) A (A (A S)) / (sum_i d_i |S_i|^2 + eps), d = A (A (A 1)), per graph, in the chain form (never A A A)."""
    zd = torch.cat([S, S.new_ones(S.shape[:-1] + (1,))], -1)
    for _ in range(3):
        zd = adj @ zd
    num = (S * zd[..., :-1]).sum(dim=(-2, -1))
    den = (zd[..., -1] * (S * S).sum(-1)).sum(-1)
    return -(num / (den + eps))


def hosc_loss_terms(adj: Optional[Tensor], S: Tensor, adj_pooled: Optional[Tensor], mask: Optional[Tensor] = None,
                    graph_sizes: Optional[Tensor] = None, alpha: float = 0.5, mu: float = 0.1, k: Optional[int] = None,
                    hosc_ortho: bool = False) -> Tensor:
    """[2,B]: per-graph ((1 - alpha) cut + alpha ho_cut) / k and mu x orthogonality of a padded batch (the values
    :class:`~tgp.poolers.HOSCPooling` averages), float32 device operands, the adjacency without a gradient.  ``k``: the
    pooler's cluster count (S's last dimension by default).  ``graph_sizes`` (this build only): real nodes per graph of a
    zero-padded batch, lets the passes skip the padding."""
    k = S.size(-1) if k is None else k
    return _HOSCTermsFn.apply(S, adj_pooled, adj, ("dense", mask, graph_sizes), _hosc_cfg(alpha, mu, k, hosc_ortho))


def hosc_sparse_loss_terms(edge_index: Tensor, edge_weight: Optional[Tensor], S: Tensor, batch: Optional[Tensor] = None,
                           alpha: float = 0.5, mu: float = 0.1, k: Optional[int] = None,
                           hosc_ortho: bool = False) -> Optional[Tensor]:
    """[2,B]: the same two rows for an un-padded batch (first-order cut with out-degrees, as
    :func:`sparse_mincut_loss`); None when the operands take the composed forms (float64, edge weights that require grad,
    an unsorted batch, no nodes or no edges).  MinCut's orthogonality row (``hosc_ortho`` False) is formed per graph from
    the segment product S_g^T S_g beside the Function."""
    w = None if edge_weight is None else check_and_filter_edge_weights(edge_weight).view(-1)
    if (not (_native_f32(S, w) and S.dim() == 2 and S.size(0) > 0 and edge_index.size(1) > 0)
            or (w is not None and w.requires_grad)):
        return None
    K.N.require_device(S, edge_index, w, batch)
    layout = _flat_layout(S, batch)
    if layout is None:
        return None
    k = S.size(1) if k is None else k
    n = S.size(0)
    native_ortho = hosc_ortho or mu == 0
    source = _hosc_csr(edge_index, w, n)
    terms = _HOSCTermsFn.apply(S, None, source, layout, _hosc_cfg(alpha, mu if native_ortho else 0.0, k, hosc_ortho))
    if native_ortho:
        return terms
    nb = layout[1].numel() - 1
    gram = _per_graph_gram(S, batch, nb)
    gram = gram / torch.norm(gram, dim=(-2, -1), keepdim=True)
    target = torch.eye(S.size(1), device=S.device, dtype=S.dtype) / math.sqrt(S.size(1))
    return torch.stack([terms[0], mu * torch.norm(gram - target, dim=(-2, -1))])


def hosc_orthogonality_loss(S: Tensor, mask: Optional[Tensor] = None, batch_reduction: str = "mean") -> Tensor:
    """HOSC's orthogonality loss (sqrt(K) - sum_j ||S_*j|| / sqrt(n)) / (sqrt(K) - 1) per graph, n = mask.sum(1) (N without
    a mask); 0 for K <= 1 (reference utils/losses.py:597-641)."""
    if S.size(-1) <= 1:
        return _reduce(S.new_zeros(S.size(0)), batch_reduction)
    if _native_f32(S) and S.dim() == 3:
        terms = _HOSCTermsFn.apply(S, None, None, ("dense", mask, None), (0.0, 1.0, 1.0, True))
        return _reduce(terms[1], batch_reduction)
    return _reduce(_hosc_ortho_composed(S, S.size(1) if mask is None else mask.sum(1)), batch_reduction)


def unbatched_hosc_orthogonality_loss(S: Tensor, batch: Optional[Tensor] = None,
                                      batch_reduction: str = "mean") -> Tensor:
    """HOSC's orthogonality loss of an un-padded batch (reference utils/losses.py:392-432): n = the graph's node count; a
    0-dim zero for K <= 1."""
    n, k = S.shape
    if k <= 1:
        return S.new_zeros(())
    layout = _flat_layout(S, batch) if _native_f32(S) and n > 0 else None
    if layout is not None:
        terms = _HOSCTermsFn.apply(S, None, None, layout, (0.0, 1.0, 1.0, True))
        return _reduce(terms[1], batch_reduction)
    nb = num_graphs_of(batch)
    bvec = _batch_or_zeros(batch, n, S.device)
    sizes = torch.bincount(bvec, minlength=nb)[:nb].to(S.dtype)
    norms = torch.stack([torch.norm(S[bvec == g], dim=0).sum() for g in range(nb)]) if nb else S.new_zeros(0)
    sqrt_k = math.sqrt(k)
    return _reduce((sqrt_k - norms / sizes.sqrt()) / (sqrt_k - 1), batch_reduction)


def sparse_ho_mincut_loss(edge_index: Tensor, S: Tensor, edge_weight: Optional[Tensor] = None,
                          batch: Optional[Tensor] = None, batch_reduction: str = "mean") -> Tensor:
    """The higher-order (motif) cut -trace(S_g^T M_g S_g) / (trace(S_g^T D_g S_g) + eps), M = A A A, D = diag(M 1), of an
    edge list, in the chain form M S = A (A (A S)), M 1 = A (A (A 1)) (reference utils/losses.py:218-316).  As there: a
    single graph gives a 0-dim value whatever the reduction, an empty edge list zeros."""
    n = S.size(0)
    nb = num_graphs_of(batch)
    w = None if edge_weight is None else check_and_filter_edge_weights(edge_weight).view(-1)
    if edge_index.numel() == 0:
        return S.new_zeros(()) if nb == 1 else _reduce(S.new_zeros(nb), batch_reduction)
    if _native_f32(S, w) and S.dim() == 2 and n > 0 and not (w is not None and w.requires_grad):
        K.N.require_device(S, edge_index, w, batch)
        layout = _flat_layout(S, batch)
        if layout is not None:
            ho = _HOSCTermsFn.apply(S, None, _hosc_csr(edge_index, w, n), layout, (1.0, 0.0, 1.0, False))[0]
            return ho[0] if nb == 1 else _reduce(ho, batch_reduction)
    bvec = _batch_or_zeros(batch, n, S.device)
    wv = torch.ones(edge_index.size(1), device=S.device, dtype=S.dtype) if w is None else w.to(S.dtype)
    src, dst = edge_index[0], edge_index[1]
    zd = torch.cat([S, S.new_ones(n, 1)], 1)
    for _ in range(3):  # A x as a gather and an index_add over the edges (duplicates add up, as coalescing does)
        zd = _seg_sum(wv.unsqueeze(-1) * zd[dst], src, n)
    num = _seg_sum((S * zd[:, :-1]).sum(-1), bvec, nb)
    den = _seg_sum(zd[:, -1] * (S * S).sum(-1), bvec, nb)
    ho = -(num / (den + eps))
    return ho[0] if nb == 1 else _reduce(ho, batch_reduction)


# ------------------------------------------------------------------------------------------------ BN-Pool
def _weighted_bce_terms(rec_adj: Tensor, adj: Tensor, mask: Optional[Tensor], balance_links: bool) -> Tensor:
    """Per-graph sums of :func:`weighted_bce_reconstruction_loss` (before normalisation and batch reduction)."""
    loss = torch.nn.functional.binary_cross_entropy_with_logits(rec_adj, adj, reduction="none")
    if balance_links:
        edge_mask = adj != 0
        if mask is not None:
            n = mask.sum(-1)
            edge_mask = edge_mask & mask.unsqueeze(-1) & mask.unsqueeze(-2)
        else:
            n = adj.shape[-1]
        n_edges = edge_mask.sum((-1, -2))
        n_not_edges = torch.clamp(n ** 2 - n_edges, min=1)
        # (integer / integer: a float32 quotient whatever the dtype of the logits, as in the reference)
        balance = (n_not_edges / torch.clamp(n_edges, min=1)).to(loss.dtype)
        # torch.where on the weight instead of the reference's loss[edge_mask] *= repeat_interleave(balance, n_edges),
        # which waits on the host for the counts
        loss = loss * torch.where(edge_mask, balance[..., None, None], loss.new_ones(()))
    if mask is not None:
        loss = loss * mask.unsqueeze(-1) * mask.unsqueeze(-2)
    return loss.sum((-1, -2))


def weighted_bce_reconstruction_loss(rec_adj: Tensor, adj: Tensor, mask: Optional[Tensor] = None,
                                     balance_links: bool = True, normalizing_const: Optional[Tensor] = None,
                                     batch_reduction: str = "mean") -> Tensor:
    """Binary cross entropy between the logits ``rec_adj`` [B,N,N] and the targets ``adj`` (any real value), over the
    entries whose row and column are in ``mask``; with ``balance_links`` the entries with ``adj != 0`` weigh
    max(n^2 - e, 1) / max(e, 1), e their number; per graph divided by ``normalizing_const`` (reference
    utils/losses.py:1268-1356).  Composed torch ops on logits that already exist: the fallback and the fp32 oracle of
    :func:`bnpool_rec_loss_terms`, which never forms them."""
    loss = _weighted_bce_terms(rec_adj, adj, mask, balance_links)
    if normalizing_const is not None:
        loss = loss / normalizing_const
    return _reduce(loss, batch_reduction)


def kl_loss(q, p, mask: Optional[Tensor] = None, batch: Optional[Tensor] = None, batch_size: int = None,
            normalizing_const: Optional[Tensor] = None, batch_reduction: str = "mean") -> Tensor:
    """KL(q || p) summed over the last axis and over the nodes of each graph (``mask`` [B,N] for a padded batch, ``batch``
    and ``batch_size`` for an un-padded one), divided by ``normalizing_const`` (reference utils/losses.py:1359-1443)."""
    if mask is not None and batch is not None:
        raise ValueError("Cannot specify both mask and batch")
    if batch is not None and batch_size is None:
        raise ValueError("Batch size must be specified if batch is specified")
    loss = torch.distributions.kl_divergence(q, p).sum(-1)
    if mask is not None:
        loss = (loss * mask).sum(-1)
    elif batch is not None:
        loss = _seg_sum(loss, batch, batch_size)
    else:
        loss = loss.sum(-1)
    if normalizing_const is not None:
        loss = loss / normalizing_const
    return _reduce(loss, batch_reduction)


def cluster_connectivity_prior_loss(K: Tensor, K_mu: Tensor, K_var: Tensor, normalizing_const: Optional[Tensor] = None,
                                    batch_reduction: str = "mean") -> Tensor:
    """Gaussian prior on BN-Pool's cluster connectivity matrix: sum (K - K_mu)^2 / (2 K_var), shared among the graphs of
    ``normalizing_const`` and divided by it (reference utils/losses.py:1446-1517)."""
    prior_loss = (0.5 * (K - K_mu) ** 2 / K_var).sum()
    if normalizing_const is not None:
        bs = normalizing_const.shape[0] if normalizing_const.dim() > 0 else 1
        prior_loss = prior_loss / bs / normalizing_const
    return _reduce(prior_loss, batch_reduction)


def sparse_bce_reconstruction_loss(link_prob_loigit, true_y, edges_batch_id: Optional[Tensor] = None, batch_size=None,
                                   batch_reduction: str = "mean"):
    """(loss, sampled-edge count): binary cross entropy over sampled edges, averaged per graph of ``edges_batch_id``
    (reference utils/losses.py:1520-1562)."""
    rec_loss = torch.nn.functional.binary_cross_entropy_with_logits(link_prob_loigit, true_y, reduction="none")
    if edges_batch_id is None:
        count = torch.tensor(rec_loss.size(0), device=rec_loss.device, dtype=rec_loss.dtype)
        return rec_loss.mean(), count
    summed_loss = _seg_sum(rec_loss, edges_batch_id, batch_size)
    summed_count = torch.clamp(_seg_sum(torch.ones_like(rec_loss), edges_batch_id, batch_size), min=1)
    return _reduce(summed_loss / summed_count, batch_reduction), summed_count


class _BNPoolRecFn(torch.autograd.Function):
    """[B] per-graph reconstruction loss of BN-Pool, rec_b = (c sum_{a != 0} bce + sum_{a == 0} bce) / n^2 over the
    logits L = S K S^T, with a native backward; neither L nor any other [B,N,N] tensor is formed.

    Forward: T = S K (torch.matmul, K / N of the work), one launch over the 32x32 logit tiles that reads the adjacency
    once, one tail launch.  Backward: two launches recompute the tiles and give P = G S and Q = G^T T for
    G = d loss / d L (the class weight c is a constant of the counts, saved from the forward); then dS = P K^T + Q and
    dK = sum_b S^T P as small products.  No float atomics: forward and backward are reproducible bit for bit.  The
    adjacency and the mask get no gradient."""

    @staticmethod
    def forward(ctx, S, Kmat, adj, mask):
        T = torch.matmul(S, Kmat)
        rec, stats = K.bnpool_rec_fwd(T, S, adj, mask)
        ctx.save_for_backward(S, Kmat, adj, stats)
        ctx.mask = mask
        return rec

    @staticmethod
    def backward(ctx, g):
        S, Kmat, adj, stats = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None
        Kc = S.size(-1)
        P, Q = K.bnpool_rec_bwd(torch.matmul(S, Kmat), S, adj, ctx.mask, g.to(torch.float32).contiguous(), stats)
        dS = dK = None
        if ctx.needs_input_grad[0]:
            dS = torch.addmm(Q.view(-1, Kc), P.view(-1, Kc), Kmat.t()).view(S.shape)
        if ctx.needs_input_grad[1]:
            dK = torch.matmul(S.reshape(-1, Kc).t(), P.view(-1, Kc))
        return dS, dK, None, None


def bnpool_rec_loss_terms(S: Tensor, K_: Tensor, adj: Tensor, mask: Optional[Tensor] = None) -> Tensor:
    """[B]: BN-Pool's reconstruction loss per graph, ``weighted_bce_reconstruction_loss(S K S^T, adj, mask,
    balance_links=True, normalizing_const=n^2, ...)`` before the batch reduction.  float32 device operands (``adj``
    without a gradient, K at most 256 clusters) run on the native route, which never forms the logits; float64 operands,
    a differentiable ``adj`` and wider K take the composed form.  float32 host tensors raise: there is no CPU fallback."""
    if (_native_f32(S, K_, adj) and S.dim() == 3 and adj.dim() == 3 and not adj.requires_grad):
        K.N.require_device(S, K_, adj, mask)
        if S.size(-1) <= K.bnpool_max_clusters():
            return _BNPoolRecFn.apply(S, K_, adj, mask)
    rec_adj = S @ K_ @ S.transpose(-1, -2)
    n = mask.sum(-1) if mask is not None else torch.tensor(adj.shape[-1], device=adj.device)
    return _weighted_bce_terms(rec_adj, adj, mask, True) / n ** 2


# ------------------------------------------------------------------------------------------------ MaxCutPool's cut loss
def maxcut_loss(scores: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor] = None,
                batch: Optional[Tensor] = None, batch_reduction: str = "mean") -> Tensor:
    r"""The auxiliary loss of :class:`~tgp.poolers.MaxCutPooling` (reference utils/losses.py maxcut_loss):
    :math:`\mathbf{z}^\top \mathbf{A} \mathbf{z} / V` per graph with :math:`V` the graph's summed edge weight (0 -> 1),
    on the list as given -- self-loops and duplicate edges count --, then the batch reduction.

    Device float32 scores with an int64 ``[2, E]`` list, a sorted (or no) batch vector, the mean reduction and edge
    weights that need no gradient take the native node (``tgp.functions.maxcut_loss``: one pass over the by-source
    groups, no sparse tensor, no sort); everything else takes the composed form below."""
    if scores.dim() == 2 and scores.size(1) == 1:
        scores = scores.squeeze(-1)
    elif scores.dim() != 1:
        raise ValueError(f"Expected scores to have shape [N] or [N, 1], got {scores.shape}")
    n = scores.size(0)
    if edge_weight is not None and edge_weight.dim() > 1:
        edge_weight = edge_weight.squeeze()
    if maxcut_loss_native_case(scores, edge_index, edge_weight, batch, batch_reduction):
        if batch is None:
            return Fn.maxcut_loss(scores, edge_index, edge_weight, None, K.maxcut_one_graph_ptr(n, scores.device), 1, n)
        from .ops import batch_info
        info = batch_info(batch)
        return Fn.maxcut_loss(scores, edge_index, edge_weight, batch, info.ptr, info.num_graphs, info.max_nodes)
    if batch is None:
        batch = torch.zeros(n, dtype=torch.long, device=scores.device)
    w = torch.ones(edge_index.size(1), dtype=scores.dtype, device=scores.device) if edge_weight is None else edge_weight
    src, dst = edge_index[0], edge_index[1]
    az = _seg_sum(w * scores[dst], src, n)
    nb = num_graphs_of(batch)
    cut = _seg_sum(scores * az, batch, nb)
    vol = _seg_sum(w, batch[src], nb)
    vol = torch.where(vol == 0, torch.ones_like(vol), vol)
    return _reduce(cut / vol, batch_reduction)


def maxcut_loss_native_case(scores: Tensor, edge_index, edge_weight: Optional[Tensor], batch: Optional[Tensor],
                            batch_reduction: str = "mean") -> bool:
    """Does :func:`maxcut_loss` take its native node for these inputs?"""
    if not (isinstance(edge_index, Tensor) and not edge_index.is_sparse and edge_index.dim() == 2
            and edge_index.size(0) == 2 and edge_index.dtype == torch.int64 and edge_index.is_cuda
            and scores.is_cuda and scores.dtype == torch.float32 and scores.numel() > 0 and batch_reduction == "mean"):
        return False
    if edge_weight is not None and (edge_weight.dtype != torch.float32 or edge_weight.numel() != edge_index.size(1)
                                    or (edge_weight.requires_grad and torch.is_grad_enabled())):
        return False
    if batch is None:
        return True
    if not (batch.is_cuda and batch.dtype == torch.int64 and batch.numel() == scores.numel()):
        return False
    from .ops import batch_info
    info = batch_info(batch)
    return bool(info.is_sorted and info.num_graphs >= 1)
