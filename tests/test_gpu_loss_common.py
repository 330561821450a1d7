"""What the dense-loss kernels share (csrc/loss_common.h): one orthogonality term behind MinCut's, DMoN's and HOSC's
loss tails, and one streaming row pass over a padded adjacency behind HOSC's matrix-vector product and DMoN's degrees.
Both against float64 compositions in torch, at the tolerances of test_gpu_losses.py (orthogonality loss and its
gradient) and the project's fp32 parity bound rtol = atol = 1e-5 (row pass)."""
import math

import pytest
import torch

from test_gpu_losses import BWD, FWD

pytestmark = pytest.mark.gpu
PARITY = dict(rtol=1e-5, atol=1e-5)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("Kc", [1, 7, 64, 130])  # 1: |Y| = 0, so W = 0; 64 and 130: the 1024-thread form
def test_one_orthogonality_term_behind_three_entry_points(dev, Kc):
    from tgp import kernels as K
    B, N = 3, 40
    g = torch.Generator().manual_seed(Kc)
    S = torch.softmax(torch.randn(B, N, Kc, generator=g), -1).to(dev)
    A = (torch.rand(B, N, N, generator=g) < 0.2).float().to(dev)
    gram = S.transpose(1, 2) @ S
    raw = S.transpose(1, 2) @ A @ S
    den = torch.ones(B, device=dev)
    sqrt_k, inv_k, alpha = math.sqrt(Kc), 1.0 / Kc, 0.5

    mc = K.mincut_loss_terms(raw, den, gram)[1]
    _, dm_part = K.dmon_dense_terms(A, S)
    dm_out, _, _, dm_stats = K.dmon_loss_terms(dm_part, raw, None, gram, sqrt_k, False, (1.0, 1.0, 1.0))
    hs_part = K.hosc_node_terms(S, None, None, None, None)
    hs_out, _, hs_stats = K.hosc_loss_terms(hs_part, Kc, raw, gram, alpha, 1.0, inv_k, False)
    assert torch.equal(mc, dm_out[2]) and torch.equal(mc, hs_out[1])

    W_mc = K.mincut_loss_terms_bwd(raw, den, gram, torch.ones(2, B, device=dev))[2]
    W_dm = K.dmon_loss_terms_bwd(torch.ones(3, B, device=dev), dm_stats, gram, Kc, sqrt_k, False, False,
                                 (1.0, 1.0, 1.0))[3]
    W_hs = K.hosc_loss_terms_bwd(torch.ones(2, B, device=dev), hs_stats, gram, Kc, alpha, 1.0, inv_k, False, False)[2]
    assert torch.equal(W_mc, W_dm) and torch.equal(W_mc, W_hs)

    G = gram.double()
    n = torch.linalg.matrix_norm(G, keepdim=True)
    Y = G / n - torch.eye(Kc, dtype=torch.float64, device=dev) / math.sqrt(Kc)
    ny = torch.linalg.matrix_norm(Y, keepdim=True)
    gy = (G * Y).sum((-2, -1), keepdim=True)
    W = torch.where(ny > 0, (Y - G * gy / (n * n)) / (ny * n), torch.zeros_like(Y))
    print(f"K={Kc}: forward max |err| {float((mc.double() - ny.view(B)).abs().max()):.3e}, "
          f"W max |err| {float((W_mc.double() - W).abs().max()):.3e}")
    torch.testing.assert_close(mc, ny.view(B).float(), **FWD)
    torch.testing.assert_close(W_mc, W.float(), **BWD)
    if Kc == 1:
        assert float(mc.abs().max()) == 0.0 and float(W_mc.abs().max()) == 0.0


# (G lanes per row, load width): 5 -> (16, element), 64 -> (16, float4), 70 and 333 -> (64, element), 132 -> (64, float4)
@pytest.mark.parametrize("N", [5, 64, 70, 132, 333])
def test_row_pass_over_adjacency(dev, N):
    from tgp import kernels as K
    B, Kc = 3, 4
    g = torch.Generator().manual_seed(N)
    A = ((torch.rand(B, N, N, generator=g) < 0.2).float() * torch.rand(B, N, N, generator=g)).to(dev)
    S = torch.softmax(torch.randn(B, N, Kc, generator=g), -1).to(dev)
    v = torch.randn(B, N, generator=g).to(dev)
    buf = torch.empty(B * N + 1, device=dev)
    v_off = buf[1:].view(B, N).copy_(v)  # contiguous, one float into its storage: not 16-byte aligned
    assert v_off.is_contiguous() and v_off.data_ptr() % 16 != 0
    sizes = torch.tensor([N, max(1, N // 2), max(1, N - 3)], device=dev)
    rows = (torch.arange(N, device=dev).unsqueeze(0) < sizes.unsqueeze(1)).double()
    mask = torch.rand(B, N, generator=g).to(dev) < 0.7
    A64, v64 = A.double(), v.double()
    deg64, Av64 = A64.sum(-1), (A64 @ v64.unsqueeze(-1)).squeeze(-1)

    ones = K.hosc_matvec(A, None)
    deg = K.dmon_dense_terms(A, S)[0]
    assert torch.equal(ones, deg)  # one kernel template, the same adds
    torch.testing.assert_close(ones, deg64.float(), **PARITY)
    torch.testing.assert_close(K.hosc_matvec(A, v), Av64.float(), **PARITY)
    torch.testing.assert_close(K.hosc_matvec(A, v_off), Av64.float(), **PARITY)
    torch.testing.assert_close(K.hosc_matvec(A, None, sizes), (deg64 * rows).float(), **PARITY)
    torch.testing.assert_close(K.hosc_matvec(A, v, sizes), (Av64 * rows).float(), **PARITY)
    torch.testing.assert_close(K.dmon_dense_terms(A, S, None, sizes)[0], (deg64 * rows).float(), **PARITY)
    torch.testing.assert_close(K.dmon_dense_terms(A, S, mask)[0], (deg64 * mask.double()).float(), **PARITY)
    torch.testing.assert_close(K.dmon_dense_terms(A, S, mask, sizes)[0], (deg64 * rows * mask.double()).float(),
                               **PARITY)
