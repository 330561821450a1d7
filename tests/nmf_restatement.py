"""NMF pooling's selector, stated once in plain torch on the CPU (reference select/nmf_select.py:58-81 and the
coordinate-descent solver scikit-learn runs for it: ``non_negative_factorization(..., solver="cd")`` with
``shuffle=False``, ``tol=1e-4`` and no regularisation).

TEST INFRASTRUCTURE ONLY.  The kernel of ``csrc/nmf.hip`` and the composed route of ``tgp/poolers/nmf.py`` are compared
against this file; it runs in float64 (the yardstick) and in float32 (the error of the reference's own arithmetic).

Per graph with ``n`` nodes and ``ka = max(1, min(K, n))``: no rows for ``n == 0``; ``eye(n)`` for ``n > 1 and ka >= n``;
``ones(n, 1)`` for ``ka == 1``; otherwise the factorisation of the clamped dense adjacency from ``W0 [n, ka]``,
``H0^T [n, ka]`` and ``S = softmax(H^T)``.  In a multi-graph batch every graph's ``S`` is right-padded to ``K`` columns.
"""
from typing import List, Optional, Tuple

import torch

_M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ the default init
def hash_uniform(seed: int, which: int, n: int, ka: int) -> torch.Tensor:
    """u [n, ka] in (0, 1] (float64, exact multiples of 2^-24): the 32-bit hash of (seed, which, local node index,
    component) of ``nmf_uniform`` in csrc/nmf.hip, written with int64 operations masked to 32 bits."""
    i = torch.arange(n, dtype=torch.int64).view(-1, 1)
    t = torch.arange(ka, dtype=torch.int64).view(1, -1)
    base = (((int(seed) & _M32) * 0x9E3779B9) + (int(which) & _M32) * 0x85EBCA6B + 0x165667B1) & _M32
    h = (base + ((i * 0xC2B2AE35) & _M32) + ((t * 0x27D4EB2F) & _M32)) & _M32
    h = h ^ (h >> 16)
    h = (h * 0x7FEB352D) & _M32
    h = h ^ (h >> 15)
    h = (h * 0x846CA68B) & _M32
    h = h ^ (h >> 16)
    return ((h >> 8) + 1).to(torch.float64) / 16777216.0


def default_init(adj: torch.Tensor, ka: int, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(W0, H0^T) [n, ka] each in ``adj``'s dtype: ``avg * 2u`` with scikit-learn's ``avg = sqrt(mean(A) / ka)``."""
    n = adj.size(0)
    avg = torch.sqrt(adj.mean() / ka)
    w0 = avg * (2.0 * hash_uniform(seed, 0, n, ka)).to(adj.dtype)
    h0t = avg * (2.0 * hash_uniform(seed, 1, n, ka)).to(adj.dtype)
    return w0, h0t


def sklearn_random_init(adj, ka: int, rng):
    """scikit-learn's ``init="random"`` (``_initialize_nmf``): (W0 [n, ka], H0 [ka, n]) in ``adj``'s numpy dtype, from a
    ``numpy.random.RandomState``."""
    import numpy as np
    avg = np.sqrt(adj.mean() / ka)
    h = avg * rng.standard_normal(size=(ka, adj.shape[1])).astype(adj.dtype, copy=False)
    w = avg * rng.standard_normal(size=(adj.shape[0], ka)).astype(adj.dtype, copy=False)
    np.abs(h, out=h)
    np.abs(w, out=w)
    return w, h


# ------------------------------------------------------------------------------------------------ the solver
def _half_sweep(a: torch.Tensor, u: torch.Tensor, f: torch.Tensor, ordered: bool) -> float:
    """One ``_update_coordinate_descent``: ``u`` [n, ka] is updated in place against ``a ~ u f^T``; returns the
    violation (added in float64, as scikit-learn's is)."""
    ka = u.size(1)
    if ordered:  # the kernel's order: every entry of both products added in ascending j, one rounded product at a time
        gram = torch.zeros(ka, ka, dtype=f.dtype)  # (elementwise operations only: the same bits on every machine,
        prod = torch.zeros(a.size(0), ka, dtype=f.dtype)  # whatever its BLAS and its thread count)
        for j in range(f.size(0)):
            gram = gram + f[j].view(-1, 1) * f[j].view(1, -1)
            prod = prod + a[:, j:j + 1] * f[j].view(1, -1)
    else:
        gram = f.t() @ f
        prod = a @ f
    viol = torch.zeros(u.size(0), dtype=torch.float64)
    for t in range(ka):
        if ordered:  # the kernel's order: -P, then the Gram row in ascending r, every product rounded on its own
            grad = -prod[:, t]
            for r in range(ka):
                grad = grad + gram[t, r] * u[:, r]
        else:
            grad = -prod[:, t] + u @ gram[t]
        ut = u[:, t].clone()
        pg = torch.where(ut == 0, grad.clamp(max=0), grad)
        viol += pg.abs().double()
        hess = gram[t, t]
        if float(hess) != 0.0:
            u[:, t] = (ut - grad / hess).clamp(min=0)
    return float(viol.sum())


def cd_nmf(a: torch.Tensor, w0: torch.Tensor, h0t: torch.Tensor, tol: float = 1e-4, max_iter: int = 5000,
           ordered: bool = False):
    """(W, H^T, n_iter, ratios) of scikit-learn's ``_fit_coordinate_descent`` on the non-negative ``a`` [n, n] from
    ``w0``, ``h0t`` [n, ka], in ``a``'s dtype; ``ratios``: violation / first violation of every iteration."""
    w, ht = w0.clone().to(a.dtype), h0t.clone().to(a.dtype)
    at = a.t().contiguous()
    ratios: List[float] = []
    vinit, n_iter = 0.0, 0
    for n_iter in range(1, int(max_iter) + 1):
        viol = _half_sweep(a, w, ht, ordered)
        viol += _half_sweep(at, ht, w, ordered)
        if n_iter == 1:
            vinit = viol
        if vinit == 0:
            ratios.append(0.0)
            break
        ratios.append(viol / vinit)
        if viol / vinit <= tol:
            break
    return w, ht, n_iter, ratios


# ------------------------------------------------------------------------------------------------ the selector
def graph_slices(batch: Optional[torch.Tensor], n: int) -> List[Tuple[int, int]]:
    if batch is None or batch.numel() == 0:
        return [(0, n)]
    sizes = torch.bincount(batch).tolist()
    out, lo = [], 0
    for s in sizes:
        out.append((lo, lo + s))
        lo += s
    return out


def dense_adjacency(ei: torch.Tensor, ew: Optional[torch.Tensor], lo: int, hi: int, dtype=torch.float32) -> torch.Tensor:
    """The graph's dense adjacency as ``to_dense_adj`` builds it: duplicates added in edge-list order in the weights'
    dtype (fp32 unless they are float64), then cast."""
    m = hi - lo
    keep = ((ei[0] >= lo) & (ei[0] < hi)).nonzero().view(-1)
    w = torch.ones(ei.size(1)) if ew is None else ew.reshape(-1)
    acc_dtype = torch.float64 if w.dtype == torch.float64 else torch.float32
    a = torch.zeros(m, m, dtype=acc_dtype)
    for e in keep.tolist():  # (edge-list order, one addition at a time)
        a[int(ei[0, e]) - lo, int(ei[1, e]) - lo] += w[e].to(acc_dtype)
    return a.to(dtype)


def nmf_select(ei: torch.Tensor, k: int, ew: Optional[torch.Tensor] = None, batch: Optional[torch.Tensor] = None,
               num_nodes: Optional[int] = None, fixed_k: bool = False, seed: int = 0, tol: float = 1e-4,
               max_iter: int = 5000, init=None, dtype=torch.float32, ordered: bool = False) -> dict:
    """The selector on CPU tensors.  ``init``: ``(W0 [N, K], H0^T [N, K])`` node-major (columns >= ka ignored) or None
    for the default init.  Returns ``s``, and per graph ``iters`` (0 where nothing is factorised), ``ratios``, and the
    raw ``w`` / ``ht`` [N, K] (zeros where nothing is factorised)."""
    n = num_nodes if num_nodes is not None else (batch.numel() if batch is not None and batch.numel() else
                                                 (int(ei.max()) + 1 if ei.numel() else 0))
    multi = batch is not None and batch.numel() > 0 and int(batch.max()) > 0
    slices = graph_slices(batch if multi else None, n)
    K = int(k)
    width = K if (multi or fixed_k) else max(1, min(K, n))
    s = torch.zeros(n, width if n else (K if fixed_k else 0), dtype=dtype)
    w_all, ht_all = torch.zeros(n, K, dtype=dtype), torch.zeros(n, K, dtype=dtype)
    iters, ratios = [], []
    for lo, hi in slices:
        m = hi - lo
        ka = max(1, min(K, m))
        if m == 0 or (m > 1 and ka >= m) or ka == 1:
            if m > 1 and ka >= m:
                s[lo:hi, :m] = torch.eye(m, dtype=dtype)
            elif m > 0:
                s[lo:hi, 0] = 1.0
            iters.append(0)
            ratios.append([])
            continue
        a = dense_adjacency(ei, ew, lo, hi, dtype).clamp(min=0)
        if init is None:
            w0, h0t = default_init(a, ka, seed)
        else:
            w0, h0t = init[0][lo:hi, :ka].to(dtype), init[1][lo:hi, :ka].to(dtype)
        w, ht, it, rs = cd_nmf(a, w0, h0t, tol, max_iter, ordered)
        s[lo:hi, :ka] = torch.softmax(ht, dim=-1)
        w_all[lo:hi, :ka], ht_all[lo:hi, :ka] = w, ht
        iters.append(it)
        ratios.append(rs)
    return {"s": s, "iters": iters, "ratios": ratios, "w": w_all, "ht": ht_all}


def planted_graphs(blocks_per_graph, seed: int, p_in: float = 0.8, p_out: float = 0.04, directed=()):
    """Seeded block graphs with weights in [0.1, 1): (edge_index, edge_weight, batch).  A graph listed in ``directed``
    keeps only a random half of each edge pair's directions (an asymmetric adjacency); an empty block list gives a graph
    without nodes."""
    g = torch.Generator().manual_seed(seed)
    eis, ews, bs, off = [], [], [], 0
    for gi, blocks in enumerate(blocks_per_graph):
        lab = torch.cat([torch.full((s,), c, dtype=torch.long) for c, s in enumerate(blocks)]) if blocks else \
            torch.zeros(0, dtype=torch.long)
        n = lab.numel()
        same = lab.view(-1, 1) == lab.view(1, -1)
        prob = torch.where(same, torch.tensor(p_in), torch.tensor(p_out))
        up = torch.triu(torch.rand(n, n, generator=g) < prob, 1)
        w = torch.triu(torch.rand(n, n, generator=g) * 0.9 + 0.1, 1) * up
        if gi in directed:
            keep = torch.rand(n, n, generator=g) < 0.5
            a = w * keep + (w * ~keep).t()
        else:
            a = w + w.t()
        idx = a.nonzero().t()
        eis.append(idx + off)
        ews.append(a[idx[0], idx[1]])
        bs.append(torch.full((n,), gi, dtype=torch.long))
        off += n
    return torch.cat(eis, 1), torch.cat(ews), torch.cat(bs)
