"""The sampled-edge loss of BN-Pool's unbatched mode without a GPU: the C entries bind from the header, the public
function has its signature, float32 host tensors are refused and float64 ones take the composed expression."""
import ctypes
import inspect

import pytest
import torch


def test_header_entries_bind_and_reject_bad_arguments():
    from tgp import _native
    assert len(_native.SIGNATURES["tgp_bnedge_fwd_f32"][1]) == 17
    assert len(_native.SIGNATURES["tgp_bnedge_bwd_f32"][1]) == 27
    lib = _native.lib()
    p = ctypes.addressof((ctypes.c_int64 * 4)())
    fwd = lambda K, status: lib.tgp_bnedge_fwd_f32(p, p, 4, K, p, None, p, 1, p, None, p, 1, p, None, None, status, None)
    assert fwd(257, p) == -1 and b"K=257" in lib.tgp_last_error()
    assert fwd(0, p) == -1
    assert fwd(8, None) == -1 and b"status" in lib.tgp_last_error()
    assert lib.tgp_bnedge_bwd_f32(p, p, 4, 8, None, p, 0, p, None, p, 1, p, None, p, 1, None, None, None, None, None, None,
                                  p, p, p, None, p, None) == -1  # no graph


def test_public_function_and_wrappers():
    from tgp import kernels
    from tgp.utils import losses
    params = [(n, q.default) for n, q in inspect.signature(losses.bnpool_sparse_rec_loss).parameters.items()]
    E = inspect.Parameter.empty
    assert params == [("S", E), ("K_", E), ("edge_index", E), ("neg_edge_index", E), ("batch", None), ("batch_size", None)]
    assert issubclass(losses._BNPoolEdgeRecFn, torch.autograd.Function)
    assert callable(kernels.bnpool_edge_fwd) and callable(kernels.bnpool_edge_bwd)


def test_host_tensors_float32_refused_float64_composed():
    from tgp import _native
    from tgp.utils.losses import bnpool_sparse_rec_loss
    s, k = torch.softmax(torch.randn(6, 3), -1), torch.randn(3, 3)
    pos, neg = torch.tensor([[0, 1, 4], [1, 2, 5]]), torch.tensor([[0, 3], [2, 5]])
    batch = torch.tensor([0, 0, 0, 1, 1, 1])
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        bnpool_sparse_rec_loss(s, k, pos, neg, batch)
    loss, count = bnpool_sparse_rec_loss(s.double(), k.double(), pos, neg, batch)
    e = torch.cat([pos, neg], 1)
    logits = ((s.double()[e[0]] @ k.double()) * s.double()[e[1]]).sum(-1)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.tensor([1., 1, 1, 0, 0]).double(),
                                                               reduction="none")
    want = (bce[[0, 1, 3]].mean() + bce[[2, 4]].mean()) / 2
    assert loss.dtype == torch.float64 and abs(float(loss - want)) < 1e-12 and count.tolist() == [3.0, 2.0]
