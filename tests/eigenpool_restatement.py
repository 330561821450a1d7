"""Float64 restatements of EigenPooling on the CPU, in two shapes.

``reference_shape``: what reference select/eigenpool_select.py, reduce/eigenpool_reduce.py, connect/eigenpool_conn.py and
lift/eigenpool_lift.py do -- a loop over graphs, a loop over clusters, a dense ``Theta [n, K H]`` per graph (column
``h K + c``), ``Theta^T X`` re-laid to ``[K, H F]``, ``Omega^T A_ext Omega`` from the dense per-graph adjacency with its
intra-cluster entries masked out.

``collapsed``: the shape the device code works in -- ``theta_modes [N, H]`` plus the node lists of the (graph, cluster)
groups, a segment sum for Reduce, a gather for Lift, and ``Omega^T A Omega`` with its diagonal set to zero for Connect.

Both take the labels as input (the reference's come from an unseeded k-means).  Written from the formulas; shares no code
with the package under test."""
import torch

EPS = 1e-8  # reference tgp/__init__.py
TINY = {torch.float32: 1.401298464324817e-45, torch.float64: 4.9406564584124654e-324}  # np.spacing(0) per dtype


def graph_slices(batch, n):
    if batch is None:
        return [(0, n)]
    sizes = torch.bincount(batch).tolist()
    out, off = [], 0
    for s in sizes:
        out.append((off, off + s))
        off += s
    return out


def dense_adjacency(edge_index, edge_weight, lo, hi, dtype=torch.float64):
    n = hi - lo
    a = torch.zeros(n, n, dtype=dtype)
    if edge_index.numel() == 0:
        return a
    keep = (edge_index[0] >= lo) & (edge_index[0] < hi)
    w = torch.ones(edge_index.size(1), dtype=dtype) if edge_weight is None else edge_weight.to(dtype)
    a.index_put_((edge_index[0, keep] - lo, edge_index[1, keep] - lo), w[keep], accumulate=True)
    return a


def laplacian(a, normalized=True, tiny=TINY[torch.float32]):
    d = a.sum(0)
    if not normalized:
        return torch.diag(d) - a
    dis = 1.0 / torch.sqrt(d + tiny)
    return torch.eye(a.size(0), dtype=a.dtype) - (dis.view(-1, 1) * a) * dis.view(1, -1)


def cluster_modes(a_cluster, num_modes, normalized=True, tiny=TINY[torch.float32]):
    """[m, H]: the first H modes of one cluster; also the ascending eigenvalues (None for a one-node cluster)."""
    m = a_cluster.size(0)
    if m == 1:
        return a_cluster[0, 0].repeat(num_modes).view(1, -1), None
    lam, u = torch.linalg.eigh(laplacian(a_cluster, normalized, tiny))
    cols = []
    for h in range(num_modes):
        v = u[:, min(h, m - 1)]
        cols.append(-v if v[0] < 0 else v)
    return torch.stack(cols, 1), lam


def postprocess_dense(a, remove_self_loops, degree_norm, edge_weight_norm):
    a = a.clone()
    if remove_self_loops:
        a.diagonal(dim1=-2, dim2=-1).zero_()
    if degree_norm:
        d = torch.sqrt(a.sum(-1, keepdim=True).clamp(min=EPS))
        a = (a / d) / d.transpose(-2, -1)
    if edge_weight_norm:
        mx = a.reshape(a.size(0), -1).abs().max(1)[0].view(-1, 1, 1)
        a = a / torch.where(mx == 0, torch.ones_like(mx), mx)
    return a


def postprocess_sparse(a, remove_self_loops, degree_norm, edge_weight_norm):
    """[B, K, K] -> the block-diagonal (edge_index, edge_weight) of the reference's sparse output."""
    B, k, _ = a.shape
    idx = a.nonzero()
    ei = torch.stack([idx[:, 0] * k + idx[:, 1], idx[:, 0] * k + idx[:, 2]])
    w = a[idx[:, 0], idx[:, 1], idx[:, 2]]
    keep = torch.ones_like(w, dtype=torch.bool)
    if remove_self_loops:
        keep &= ei[0] != ei[1]
    keep &= w.abs() > EPS
    ei, w = ei[:, keep], w[keep]
    if degree_norm:
        deg = torch.zeros(B * k, dtype=w.dtype).index_add_(0, ei[0], w).clamp(min=EPS)
        w = w * deg.pow(-0.5)[ei[0]] * deg.pow(-0.5)[ei[1]]
    if edge_weight_norm and w.numel():
        eb = ei[0] // k
        mx = torch.zeros(B, dtype=w.dtype).scatter_reduce_(0, eb, w.abs(), "amax", include_self=True)
        w = w / torch.where(mx == 0, torch.ones_like(mx), mx)[eb]
    return ei, w


def _post(a, opts):
    rsl, dn, ewn, sparse = (opts.get("remove_self_loops", True), opts.get("degree_norm", True),
                            opts.get("edge_weight_norm", False), opts.get("sparse_output", False))
    return postprocess_sparse(a, rsl, dn, ewn) if sparse else postprocess_dense(a, rsl, dn, ewn)


def reference_shape(x, edge_index, edge_weight, batch, labels, width, num_modes, normalized=True, opts=None,
                    dtype=torch.float64, tiny=TINY[torch.float32]):
    """dict(theta=[per-graph Theta], x_pool [B, K, H F], adj (dense [B, K, K] or (edge_index, edge_weight)), lift [N, F])."""
    x = x.to(dtype)
    thetas, pools, adjs, lifts = [], [], [], []
    for lo, hi in graph_slices(batch, x.size(0)):
        a = dense_adjacency(edge_index, edge_weight, lo, hi, dtype)
        lab = labels[lo:hi]
        theta = torch.zeros(hi - lo, width * num_modes, dtype=dtype)
        for c in range(width):
            nodes = (lab == c).nonzero().view(-1)
            if nodes.numel() == 0:
                continue
            modes, _ = cluster_modes(a[nodes][:, nodes], num_modes, normalized, tiny)
            for h in range(num_modes):
                theta[nodes, h * width + c] = modes[:, h]
        raw = theta.t() @ x[lo:hi]  # [H K, F], mode-major
        pool = raw.view(num_modes, width, -1).permute(1, 0, 2).reshape(width, -1)
        omega = torch.nn.functional.one_hot(lab, width).to(dtype)
        a_ext = a * (lab.view(-1, 1) != lab.view(1, -1)).to(dtype)
        thetas.append(theta)
        pools.append(pool)
        adjs.append(omega.t() @ a_ext @ omega)
        lifts.append(theta @ pool.view(width, num_modes, -1).permute(1, 0, 2).reshape(num_modes * width, -1))
    return dict(theta=thetas, x_pool=torch.stack(pools), adj=_post(torch.stack(adjs), opts or {}), lift=torch.cat(lifts))


def collapsed(x, edge_index, edge_weight, batch, labels, width, num_modes, normalized=True, opts=None,
              dtype=torch.float64, tiny=TINY[torch.float32]):
    """The same results from the compact form; also theta_modes [N, H], theta_ptr [B K + 1] and theta_perm [N]."""
    x = x.to(dtype)
    n = x.size(0)
    b = torch.zeros(n, dtype=torch.long) if batch is None else batch
    B = int(b.max()) + 1
    gid = b * width + labels
    G = B * width
    perm = torch.sort(gid, stable=True)[1]
    ptr = torch.zeros(G + 1, dtype=torch.long)
    ptr[1:] = torch.bincount(gid, minlength=G).cumsum(0)
    w = torch.ones(edge_index.size(1), dtype=dtype) if edge_weight is None else edge_weight.to(dtype)
    modes = torch.zeros(n, num_modes, dtype=dtype)
    loc = torch.zeros(n, dtype=torch.long)
    for g in range(G):
        nodes = perm[ptr[g]:ptr[g + 1]]
        m = nodes.numel()
        if m == 0:
            continue
        loc[nodes] = torch.arange(m)
        e = ((gid[edge_index[0]] == g) & (gid[edge_index[1]] == g)).nonzero().view(-1)
        a = torch.zeros(m, m, dtype=dtype).index_put_((loc[edge_index[0, e]], loc[edge_index[1, e]]), w[e], accumulate=True)
        modes[nodes] = cluster_modes(a, num_modes, normalized, tiny)[0]
    feat = x.size(1)
    pool = torch.zeros(G, num_modes, feat, dtype=dtype).index_add_(0, gid, modes.unsqueeze(2) * x.unsqueeze(1))
    lift = (modes.unsqueeze(2) * pool[gid]).sum(1)
    # Omega^T A Omega on the (graph, cluster) ids, minus its diagonal
    full = torch.zeros(G, G, dtype=dtype).index_put_((gid[edge_index[0]], gid[edge_index[1]]), w, accumulate=True)
    blocks = torch.stack([full[i * width:(i + 1) * width, i * width:(i + 1) * width] for i in range(B)])
    blocks = blocks * (1.0 - torch.eye(width, dtype=dtype))
    return dict(theta_modes=modes, theta_ptr=ptr, theta_perm=perm, x_pool=pool.view(B, width, num_modes * feat),
                adj=_post(blocks, opts or {}), lift=lift)


def theta_from_modes(modes, labels, batch, width):
    """The reference-shaped Theta (a list over graphs) of a compact pooling matrix."""
    n, H = modes.shape
    cols = labels.view(-1, 1) + torch.arange(H).view(1, -1) * width
    theta = torch.zeros(n, width * H, dtype=modes.dtype).scatter_(1, cols, modes)
    return [theta[lo:hi] for lo, hi in graph_slices(batch, n)]
