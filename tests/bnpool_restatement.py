"""BN-Pool's forward and losses restated with plain torch ops in any floating dtype (reference select/dp_select.py:107-137,
poolers/bnpool.py:359-447, utils/losses.py:1268-1517).  The logits S K S^T are multiplied out, [B,N,N]: this is what the
native route (csrc/bnpool.hip) never does, and the oracle it is compared with -- float64 for values and gradients,
float32 for the error an honest fp32 implementation makes on the same data.

No import from the package under test.  ``tests/test_bnpool_restatement.py`` pins these forms to the reference's own
results (tests/golden/golden_bnpool_v1.pt).

One quirk of the reference is kept, because its float64 results carry it: the class weight c = max(n^2 - e, 1) /
max(e, 1) is a quotient of two integer tensors, which torch forms in float32 whatever the dtype of the logits."""
import torch
import torch.nn.functional as F
from torch.distributions import Beta, kl_divergence

ACTS = {None: None, "relu": torch.relu, "ReLU": torch.relu}


def selector_params(x, weights, biases, act=None):
    """(alpha, beta) of the sticks' Beta posteriors: the MLP, softplus, a clamp to [1e-3, 1e3], split in two."""
    h = x
    for i, (w, b) in enumerate(zip(weights, biases)):
        h = h @ w.t() + (0 if b is None else b)
        if i + 1 < len(weights) and ACTS[act] is not None:
            h = ACTS[act](h)
    out = torch.clamp(F.softplus(h), min=1e-3, max=1e3)
    half = out.size(-1) // 2
    return out[..., :half], out[..., half:]


def sticks_to_s(z, mask=None):
    """pi_k = z_k prod_{j<k} (1 - z_j), pi_K = prod_j (1 - z_j), formed in log space; zero on masked-out rows."""
    pad = z.new_zeros(z.shape[:-1] + (1,))
    log_pi = torch.cat([torch.log(z), pad], -1) + torch.cat([pad, torch.cumsum(torch.log(1 - z), -1)], -1)
    s = torch.exp(log_pi)
    return s if mask is None else s * mask.unsqueeze(-1)


def node_counts(adj, mask):
    if mask is not None:
        return mask.sum(-1)
    return torch.full((adj.size(0),), adj.size(-1), dtype=torch.long, device=adj.device)


def rec_terms_from_logits(logits, adj, mask=None, balance=True):
    """[B]: sum over the entries inside the mask of w_ij bce(l_ij, a_ij), w = c where a != 0 (``balance``), else 1."""
    pair = torch.ones_like(adj, dtype=torch.bool) if mask is None else mask.unsqueeze(-1) & mask.unsqueeze(-2)
    bce = torch.clamp(logits, min=0) - logits * adj + torch.log1p(torch.exp(-logits.abs()))
    edge = (adj != 0) & pair
    w = torch.ones_like(logits)
    if balance:
        n = node_counts(adj, mask)
        e = edge.sum((-1, -2))
        c = (torch.clamp(n * n - e, min=1) / torch.clamp(e, min=1)).to(logits.dtype)  # (a float32 quotient: see above)
        w = torch.where(edge, c[:, None, None], w)
    return (w * bce * pair).sum((-1, -2))


def rec_terms(s, k_mat, adj, mask=None):
    """[B]: the reconstruction loss per graph, the logits S K S^T multiplied out, divided by n^2."""
    n = node_counts(adj, mask)
    return rec_terms_from_logits(s @ k_mat @ s.transpose(-1, -2), adj, mask) / (n * n)


def kl_terms(alpha, beta, alpha_prior, beta_prior, mask=None):
    """[B]: KL(Beta(alpha, beta) || Beta(alpha_prior, beta_prior)) summed over the sticks and a graph's nodes."""
    kl = kl_divergence(Beta(alpha, beta), Beta(alpha_prior, beta_prior)).sum(-1)
    return (kl if mask is None else kl * mask).sum(-1)


def prior_term(k_mat, k_mu, k_var):
    return (0.5 * (k_mat - k_mu) ** 2 / k_var).sum()


def bnpool_losses(s, k_mat, adj, mask, alpha, beta, alpha_prior, beta_prior, k_mu, k_var, eta=1.0, train_K=True):
    """The three losses of the batched mode from (S, K, A, mask, alpha, beta) and the priors."""
    n = node_counts(adj, mask)
    n2 = n * n
    out = {"quality": rec_terms(s, k_mat, adj, mask).mean(),
           "kl": eta * (kl_terms(alpha, beta, alpha_prior, beta_prior, mask) / n2).mean()}
    if train_K:
        out["K_prior"] = (prior_term(k_mat, k_mu, k_var) / n.numel() / n2).mean()
    else:
        out["K_prior"] = torch.zeros((), dtype=torch.float32, device=s.device)
    return out


def sparse_losses(s, k_mat, edge_index, neg_edge_index, batch, num_graphs, alpha, beta, alpha_prior, beta_prior, k_mu,
                  k_var, eta=1.0, train_K=True):
    """The three losses of the unbatched mode: positives the edge list, negatives ``neg_edge_index``."""
    edges = torch.cat([edge_index, neg_edge_index], 1)
    logits = ((s[edges[0]] @ k_mat) * s[edges[1]]).sum(-1)
    y = torch.cat([logits.new_ones(edge_index.size(1)), logits.new_zeros(neg_edge_index.size(1))])
    bce = torch.clamp(logits, min=0) - logits * y + torch.log1p(torch.exp(-logits.abs()))
    kl = kl_divergence(Beta(alpha, beta), Beta(alpha_prior, beta_prior)).sum(-1)
    if batch is None:
        rec, count = bce.mean(), logits.new_tensor(float(bce.numel()))
        kl_g, prior = kl.sum(-1) / count, prior_term(k_mat, k_mu, k_var) / count
    else:
        eb = batch[edges[0]]
        count = torch.clamp(logits.new_zeros(num_graphs).index_add_(0, eb, torch.ones_like(bce)), min=1)
        rec = (logits.new_zeros(num_graphs).index_add_(0, eb, bce) / count).mean()
        kl_g = (logits.new_zeros(num_graphs).index_add_(0, batch, kl) / count).mean()
        prior = (prior_term(k_mat, k_mu, k_var) / num_graphs / count).mean()
    return {"quality": rec, "kl": eta * kl_g,
            "K_prior": prior if train_K else torch.zeros((), dtype=torch.float32, device=s.device)}


def dense_adjacency(edge_index, edge_weight, batch, num_nodes, transpose, dtype=torch.float32):
    """([B,Nmax,Nmax] adjacency, [B,Nmax] mask) of a sorted batch; duplicates add up; A^T when ``transpose``."""
    if batch is None:
        batch = torch.zeros(num_nodes, dtype=torch.long, device=edge_index.device)
    sizes = torch.bincount(batch)
    ptr = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])
    nb, nmax = sizes.numel(), int(sizes.max())
    w = torch.ones(edge_index.size(1), dtype=dtype) if edge_weight is None else edge_weight.to(dtype)
    g = batch[edge_index[0]]
    adj = torch.zeros(nb, nmax, nmax, dtype=dtype)
    adj.index_put_((g, edge_index[0] - ptr[g], edge_index[1] - ptr[g]), w, accumulate=True)
    mask = torch.arange(nmax).unsqueeze(0) < sizes.unsqueeze(1)
    return (adj.transpose(1, 2).contiguous() if transpose else adj), mask
