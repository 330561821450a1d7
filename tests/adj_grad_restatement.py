"""Closed form of the dense poolers' adjacency gradient (DiffPool, MinCut; padded batch, dense A handed in), in torch on
the host, in the dtype of its operands.  What csrc/dense_adj_grad.hip computes in float32; pinned against the float64
autograd of the oracle by tests/test_adj_grad_restatement.py.

Per graph b, with S [N,K] (padded rows zero), A [N,N], R = S^T A S and g_R the gradient that reaches R from the
post-processing and from an upstream gradient of R itself:

    dA_b = S_b M_b S_b^T + gamma_b q_b 1^T + c A_b

    MinCut    (cut = mean_b -trace(R_b) / (den_b + eps), den_b = sum_i d_i |s_i|^2, d = A 1; losses.py:39-56):
              M_b = g_R - (g_b / (den_b + eps)) I,   gamma_b = g_b trace(R_b) / (den_b + eps)^2,   q_i = |s_i|^2,
              g_b = the upstream gradient of graph b's term (g_cut / B for the batch mean)
    DiffPool  (link = link_scale ||A - S S^T||_F over the WHOLE batch; losses.py:644-652):
              c = g_link link_scale / ||A - S S^T||_F (0 where the norm is 0: torch.norm's subgradient),
              M_b = g_R - c I      (the -S S^T part of the residual), and the A part is c A_b.

The orthogonality and entropy losses and the pooled features do not depend on A.  ``adj_transpose`` acts in the
post-processing only (a dense input is never transposed), so it is inside g_R."""
import torch

EPS = 1e-8  # tgp/__init__.py:6 (the oracle's EPS)


def post_backward(raw, g_post, remove_self_loops, degree_norm, adj_transpose):
    """g_R from an upstream gradient of the post-processed pooled adjacency: autograd over the oracle's K x K
    post-processing alone (utils/ops.py:282-335), R a leaf."""
    import tgp_oracle as O
    leaf = raw.detach().clone().requires_grad_(True)
    post = O.postprocess_dense(leaf, remove_self_loops, degree_norm, adj_transpose, False)
    if not post.requires_grad:
        return torch.zeros_like(raw)
    (g,) = torch.autograd.grad(post, [leaf], g_post.to(raw.dtype), allow_unused=True)
    return torch.zeros_like(raw) if g is None else g


def coefficients(s, adj, g_r=None, g_cut=None, g_link=None, link_scale=1.0, eps=EPS):
    """(M [B,K,K], gamma [B], c 0-dim) of the closed form.  g_r [B,K,K] or None; g_cut [B] or None: the upstream gradient
    of every graph's cut term; g_link 0-dim or None: that of the link loss."""
    B, N, K = s.shape
    m = torch.zeros(B, K, K, dtype=s.dtype) if g_r is None else g_r.to(s.dtype).clone()
    gamma = torch.zeros(B, dtype=s.dtype)
    c = torch.zeros((), dtype=s.dtype)
    eye = torch.eye(K, dtype=s.dtype)
    if g_cut is not None:
        raw = s.transpose(1, 2) @ adj @ s
        num = torch.einsum("bii->b", raw)
        den = (adj.sum(-1) * (s * s).sum(-1)).sum(-1) + eps
        g = g_cut.to(s.dtype)
        m = m - (g / den).view(B, 1, 1) * eye
        gamma = g * num / (den * den)
    if g_link is not None:
        norm = torch.linalg.vector_norm(adj - s @ s.transpose(1, 2))
        if float(norm) > 0:
            c = g_link.to(s.dtype) * link_scale / norm
        m = m - c * eye
    return m, gamma, c


def adj_grad_from(s, adj, m, gamma, c):
    """dA from the coefficients: the N^2 K product and its rank-one and elementwise terms."""
    q = (s * s).sum(-1)
    return s @ m @ s.transpose(1, 2) + (gamma.view(-1, 1) * q).unsqueeze(-1) + c * adj


def adj_grad(s, adj, g_r=None, g_cut=None, g_link=None, link_scale=1.0, eps=EPS):
    return adj_grad_from(s, adj, *coefficients(s, adj, g_r, g_cut, g_link, link_scale, eps))


# ------------------------------------------------------------------------------------------------ case data (tests)
def make_inputs(B, N, K, F, seed, sizes=None, hidden=None, density=0.5):
    """A padded dense batch on the host: x [B,N,F], a NON-symmetric non-negative adj [B,N,N] (entries in the padding
    too: they take part in the row sums and in the link norm), a bool mask from ``sizes`` (None: no mask) and the
    selector's Linear layers [F -> (hidden ->) K] (torch.nn.Linear's range times 2: a less uniform S).  A one-node graph
    keeps a self loop, so its pooled degrees stay above the post-processing's clamp."""
    import math
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, F, generator=g)
    adj = torch.rand(B, N, N, generator=g) * (torch.rand(B, N, N, generator=g) < density)
    mask = None
    if sizes is not None:
        assert len(sizes) == B and max(sizes) <= N
        mask = torch.arange(N).unsqueeze(0) < torch.tensor(sizes).unsqueeze(1)
        for b, n in enumerate(sizes):
            if n == 1:
                adj[b, 0, 0] = 0.75
    chans = [F] + ([hidden] if hidden else []) + [K]
    ws, bs = [], []
    for fin, fout in zip(chans[:-1], chans[1:]):
        lim = 2.0 / math.sqrt(fin)
        ws.append((torch.rand(fout, fin, generator=g) * 2 - 1) * lim)
        bs.append((torch.rand(fout, generator=g) * 2 - 1) * lim)
    return x, adj, mask, ws, bs


def oracle_run(alias, x, adj, mask, ws, bs, dtype, hidden=False, **cfg):
    """The oracle on fresh leaves of ``dtype``: (outputs by path name, leaves by name, S)."""
    import tgp_oracle as O
    def leaf(t):  # (a copy: .to() of a tensor that already has the dtype is the tensor itself)
        return t.detach().to(dtype, copy=True).requires_grad_(True)
    lv = {"x": leaf(x), "adj": leaf(adj)}
    for i, (w, b) in enumerate(zip(ws, bs)):
        lv[f"W{i}"], lv[f"b{i}"] = leaf(w), leaf(b)
    ref = O.dense_pool(alias, lv["x"], lv["adj"], None, None, [lv[f"W{i}"] for i in range(len(ws))],
                       [lv[f"b{i}"] for i in range(len(bs))], act="tanh" if hidden else None, mask=mask, **cfg)
    outs = {"x": ref["x"], "adj": ref["edge_index"]}
    for i, (n, v) in enumerate(ref["loss"].items()):
        outs[f"loss{i + 1}:{n}"] = v
    return outs, lv, ref["s"]
