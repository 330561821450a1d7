"""The two float64 restatements of EigenPooling (tests/eigenpool_restatement.py) against the reference's stored results
(tests/golden/golden_eigenpool_v1.pt), and the Connect identity the device code relies on.  CPU only."""
import os

import pytest
import torch

import eigenpool_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
BLOB = torch.load(os.path.join(HERE, "golden", "golden_eigenpool_v1.pt"), weights_only=True)
CASES, OPTS = BLOB["cases"], BLOB["opts"]
TOL = dict(rtol=1e-5, atol=1e-5)


def run(fn, c, opts):
    i, cfg = c["inputs"], c["cfg"]
    return fn(i["x"], i["edge_index"], i["edge_weight"], i["batch"], c["labels"], c["width"], cfg["num_modes"],
              cfg["normalized"], opts)


def check_adj(got, want):
    if "dense" in want:
        torch.testing.assert_close(got, want["dense"].double(), **TOL)
    else:
        assert torch.equal(got[0], want["edge_index"])
        torch.testing.assert_close(got[1], want["edge_weight"].double(), **TOL)


def test_the_fixture_holds_the_group_sizes_the_issue_asks_for():
    sizes = torch.cat([c["group_sizes"] for c in CASES.values()])
    assert (sizes == 1).any() and (sizes == 2).any() and ((sizes > 2) & (sizes < 5)).any() and (sizes > 16).any()
    assert (sizes == 0).any()
    per_graph = torch.bincount(CASES["eig_batch6"]["inputs"]["batch"]).tolist()
    assert sorted(per_graph) == [3, 9, 14, 14, 20, 33]
    assert sum(c["kind"] == "sklearn" and c["ref_matches_planted"] for c in CASES.values()) >= 3


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("shape", ["reference_shape", "collapsed"])
def test_restatement_reproduces_the_reference(name, shape):
    c = CASES[name]
    for which, tol in (("f64", TOL), ("expected", TOL)):
        e = c[which]
        for oi, opts in enumerate(OPTS):
            r = run(getattr(R, shape), c, opts)
            check_adj(r["adj"], {k: v for k, v in e["adj"][oi].items()})
        theta = r["theta"] if shape == "reference_shape" else R.theta_from_modes(
            r["theta_modes"], c["labels"], c["inputs"]["batch"], c["width"])
        for t, want in zip(theta, e["theta"]):
            torch.testing.assert_close(t, want.double(), **tol)
        torch.testing.assert_close(r["x_pool"].reshape(e["x_pool"].shape), e["x_pool"].double(), **tol)
        torch.testing.assert_close(r["lift"], e["lift"].double(), **tol)


@pytest.mark.parametrize("name", sorted(CASES))
def test_compact_form_is_the_dense_theta(name):
    c = CASES[name]
    r = run(R.collapsed, c, OPTS[0])
    n, width, H = c["labels"].numel(), c["width"], c["cfg"]["num_modes"]
    b = torch.zeros(n, dtype=torch.long) if c["inputs"]["batch"] is None else c["inputs"]["batch"]
    gid = b * width + c["labels"]
    assert torch.equal(torch.bincount(gid, minlength=r["theta_ptr"].numel() - 1), c["group_sizes"])
    for g in range(r["theta_ptr"].numel() - 1):  # ascending nodes of exactly this group
        nodes = r["theta_perm"][r["theta_ptr"][g]:r["theta_ptr"][g + 1]]
        assert torch.equal(nodes, (gid == g).nonzero().view(-1))
    dense = torch.cat(c["f64"]["theta"])
    assert int((dense != 0).sum(1).max()) <= H  # at most H non-zeros per row of the reference's Theta
    x = c["inputs"]["x"].double().requires_grad_(True)
    pool = R.collapsed(x, c["inputs"]["edge_index"], c["inputs"]["edge_weight"], c["inputs"]["batch"], c["labels"], width,
                       H, c["cfg"]["normalized"], OPTS[0])["x_pool"]
    (g,) = torch.autograd.grad((pool ** 2).sum(), x)
    torch.testing.assert_close(g, c["f64"]["grad_x"], rtol=1e-9, atol=1e-10)


def test_connect_identity_with_intra_cluster_edges_and_self_loops():
    """Omega^T A_ext Omega == Omega^T A Omega with its diagonal set to zero, for a hard Omega: intra-cluster edges and
    self-loops reach only the diagonal.  Checked with remove_self_loops=False, where the diagonal must still be zero."""
    g = torch.Generator().manual_seed(3)
    n, k = 17, 4
    labels = torch.randint(0, k, (n,), generator=g)
    a = torch.rand(n, n, generator=g, dtype=torch.float64) * (torch.rand(n, n, generator=g) < 0.5)  # directed, dense-ish
    a = a + torch.diag(torch.rand(n, generator=g, dtype=torch.float64) + 0.5)  # a self-loop on every node
    same = labels.view(-1, 1) == labels.view(1, -1)
    assert bool((a * same).fill_diagonal_(0).abs().sum() > 0)  # there are intra-cluster edges beside the loops
    omega = torch.nn.functional.one_hot(labels, k).double()
    ext = omega.t() @ (a * (~same)) @ omega
    full = omega.t() @ a @ omega
    assert bool(full.diagonal().abs().min() > 0)
    torch.testing.assert_close(ext, full * (1 - torch.eye(k, dtype=torch.float64)), rtol=1e-12, atol=1e-12)
    assert float(ext.diagonal().abs().max()) == 0.0
    idx = a.nonzero().t()
    opts = dict(remove_self_loops=False, degree_norm=True, edge_weight_norm=True, sparse_output=False)
    x = torch.randn(n, 3, generator=g, dtype=torch.float64)
    r1 = R.reference_shape(x, idx, a[idx[0], idx[1]], None, labels, k, 2, True, opts)
    r2 = R.collapsed(x, idx, a[idx[0], idx[1]], None, labels, k, 2, True, opts)
    torch.testing.assert_close(r1["adj"], r2["adj"], rtol=1e-12, atol=1e-12)
    assert float(r2["adj"].diagonal(dim1=-2, dim2=-1).abs().max()) == 0.0
