"""Just Balance pooling's public surface on the CPU: the reference's names, signatures and defaults
(poolers/just_balance.py:83-100, 244-322; utils/losses.py:553-558, 1013-1020), the kind tuples that steer the routes, the
composed loss forms and the pooler's loss methods against the reference's values (tests/golden/golden_jb_v1.pt) at
rtol = atol = 1e-5 in float32 and 1e-10 in float64, the NaN error, and the argument checks of the two entry points."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jb_restatement as R  # noqa: E402
from test_jb_restatement import function_values  # noqa: E402

CASES = torch.load(os.path.join(HERE, "golden", "golden_jb_v1.pt"), weights_only=True)["cases"]
POOL = sorted(k for k, v in CASES.items() if v["kind"] == "pool")
EMPTY = inspect.Parameter.empty


def _pooler(case, dtype=torch.float32):
    from tgp.poolers import JustBalancePooling
    p = JustBalancePooling(**case["cfg"], batched=case["alias"] == "jb").to(dtype)
    p.load_state_dict({k: v.to(dtype) for k, v in case["params"].items()})
    return p


def test_constructor_and_methods_match_the_reference():
    from tgp.poolers import JustBalancePooling
    want = [("in_channels", EMPTY), ("k", EMPTY), ("act", None), ("dropout", 0.0), ("normalize_loss", True),
            ("loss_coeff", 1.0), ("remove_self_loops", True), ("degree_norm", True), ("edge_weight_norm", False),
            ("adj_transpose", True), ("lift", "precomputed"), ("s_inv_op", "transpose"), ("batched", True),
            ("sparse_output", False), ("cache_preprocessing", False)]
    got = [(n, p.default) for n, p in inspect.signature(JustBalancePooling.__init__).parameters.items() if n != "self"]
    assert got == want

    def params(fn):
        return [(n, p.default) for n, p in inspect.signature(fn).parameters.items() if n != "self"]
    assert params(JustBalancePooling.compute_loss) == [("S", EMPTY), ("mask", None), ("num_nodes", None),
                                                       ("num_supernodes", None)]
    assert params(JustBalancePooling.compute_sparse_loss) == [("S", EMPTY), ("batch", EMPTY)]
    assert JustBalancePooling.data_transforms() is None  # (the reference's NormalizeAdj lives in its tgp.data)
    p = JustBalancePooling(in_channels=5, k=4, loss_coeff=0.5, batched=False)
    assert p.extra_repr_args() == {"batched": False, "loss_coeff": 0.5, "normalize_loss": True}


def test_exports_alias_set_and_loss_signatures():
    import tgp.poolers as P
    assert "JustBalancePooling" in P.pooler_classes and "JustBalancePooling" in P.__all__
    assert P.pooler_classes == sorted(P.pooler_classes)
    assert sorted(P.pooler_map) == ["diff", "graclus", "mincut", "ndp", "topk"]  # no "jb" alias yet
    with pytest.raises(ValueError, match="Unknown pooler_name"):
        P.get_pooler("jb", in_channels=5, k=4)
    from tgp.utils import losses
    assert [(n, p.default) for n, p in inspect.signature(losses.just_balance_loss).parameters.items()] == [
        ("S", EMPTY), ("mask", None), ("normalize_loss", True), ("num_nodes", None), ("num_supernodes", None),
        ("batch_reduction", "mean")]
    assert [(n, p.default) for n, p in inspect.signature(losses.unbatched_just_balance_loss).parameters.items()] == [
        ("S", EMPTY), ("batch", None), ("normalize_loss", True), ("batch_reduction", "mean")]
    assert callable(losses.jb_loss_terms) and callable(losses.jb_loss_mean) and issubclass(losses._JBTermsFn, torch.autograd.Function)
    from tgp import kernels as K
    assert callable(K.jb_terms) and callable(K.jb_ds)


def test_loss_kind_steers_the_routes():
    from tgp.poolers import JustBalancePooling, _DenseMLPPooling
    p = JustBalancePooling(in_channels=5, k=4)
    assert p._loss_kind == "jb" and not p._wants_raw and not p._mincut_terms
    assert "jb" in _DenseMLPPooling._LOSS_ONLY_KINDS and p._loss_only  # (the one-node training functions decline it)
    assert "jb" not in _DenseMLPPooling._DENSE_ADJ_LOSS_KINDS and not p._loss_reads_dense_adj
    for name in ("jb_batched_mlp2_w", "jb_u_single_graph"):
        c = CASES[name]
        assert sorted(_pooler(c).state_dict()) == sorted(c["params"]), name


@pytest.mark.parametrize("tag,dtype,tol", [("f32", torch.float32, 1e-5), ("f64", torch.float64, 1e-10)])
def test_public_functions_on_host_tensors(tag, dtype, tol):
    from tgp.utils.losses import jb_loss_terms, just_balance_loss, unbatched_just_balance_loss
    c = CASES[f"jb_functions_{tag}"]
    i, e = c["inputs"], c["expected"]

    def dense(s, mask=None, normalize=True, num_nodes=None, num_supernodes=None):
        return jb_loss_terms(s, mask, None, None, normalize, num_nodes, num_supernodes)

    def flat(s, batch=None, normalize=True):
        return jb_loss_terms(s, batch=batch, normalize_loss=normalize)
    got = function_values(i, dense, flat)
    got_public = {
        "mask": just_balance_loss(i["s"], i["mask"]),
        "dirty_mask_sum": just_balance_loss(i["s_dirty"], i["mask"], batch_reduction="sum"),
        "mask_nonorm": just_balance_loss(i["s"], i["mask"], normalize_loss=False),
        "mask_n5_k6": just_balance_loss(i["s"], i["mask"], num_nodes=5, num_supernodes=6),
        "nomask_n5_k6": just_balance_loss(i["s"], None, True, 5, 6),
        "unbatched": unbatched_just_balance_loss(i["s_flat"], i["batch"]),
        "unbatched_nobatch": unbatched_just_balance_loss(i["s_flat"]),
        "unbatched_sum": unbatched_just_balance_loss(i["s_flat"], i["batch"], batch_reduction="sum"),
    }
    assert set(got) == set(e)
    for k, v in list(got.items()) + list(got_public.items()):
        assert v.dtype == dtype, k
        torch.testing.assert_close(v, e[k], rtol=tol, atol=tol, msg=lambda m: f"{tag}.{k}: {m}")
    # an unsorted batch vector: the same graphs, rows shuffled
    perm = torch.randperm(i["batch"].numel(), generator=torch.Generator().manual_seed(0))
    v = unbatched_just_balance_loss(i["s_flat"][perm], i["batch"][perm])
    torch.testing.assert_close(v, e["unbatched"], rtol=tol, atol=tol)
    with pytest.raises(ValueError, match="Batch reduction"):
        just_balance_loss(i["s"], batch_reduction="max")


@pytest.mark.parametrize("name", POOL)
def test_pooler_loss_methods_on_host_tensors(name):
    """compute_loss / compute_sparse_loss on the reference's own S (float32, 1e-5) and on the float64 restatement's S
    against the reference's float64 run (1e-10)."""
    c = CASES[name]
    so = c["expected"]["so"]
    p = _pooler(c)
    if c["alias"] == "jb":
        got = p.compute_loss(so["s"], so.get("in_mask"), so["num_nodes"], so["num_supernodes"])
    else:
        got = p.compute_sparse_loss(so["s"], c["inputs"].get("batch"))
    assert list(got) == ["balance_loss"] and got["balance_loss"].dim() == 0
    torch.testing.assert_close(got["balance_loss"], c["expected"]["loss"]["balance_loss"], rtol=1e-5, atol=1e-5)
    with torch.no_grad():
        _, s64, _ = R.pool_losses(c, torch.float64)
    p64 = _pooler(c, torch.float64)
    if c["alias"] == "jb":
        mask = so.get("in_mask")
        got = p64.compute_loss(s64, mask, s64.size(-2), s64.size(-1))
    else:
        got = p64.compute_sparse_loss(s64, c["inputs"].get("batch"))
    assert got["balance_loss"].dtype == torch.float64
    torch.testing.assert_close(got["balance_loss"], c["f64"]["losses"]["balance_loss"], rtol=1e-10, atol=1e-10)


def test_composed_form_differentiates_and_a_zero_column_gets_no_gradient():
    from tgp.utils.losses import just_balance_loss
    s = CASES["jb_functions_f64"]["inputs"]["s"].clone().requires_grad_(True)
    just_balance_loss(s, CASES["jb_functions_f64"]["inputs"]["mask"]).backward()
    assert torch.isfinite(s.grad).all() and bool((s.grad[:, :, 2] == 0).all()) and float(s.grad.abs().sum()) > 0


def test_nan_assignment_raises():
    from tgp.poolers import JustBalancePooling
    s = torch.softmax(torch.randn(2, 6, 4), -1)
    s[1, 2, 3] = float("nan")
    with pytest.raises(ValueError, match="Loss is NaN"):
        JustBalancePooling(in_channels=5, k=4).compute_loss(s)
    with pytest.raises(ValueError, match="Loss is NaN"):
        JustBalancePooling(in_channels=5, k=4, batched=False).compute_sparse_loss(s[1], None)


def test_an_empty_graph_gives_minus_infinity_as_the_composed_reference_does():
    from tgp.utils.losses import just_balance_loss
    s = torch.softmax(torch.randn(2, 5, 3, dtype=torch.float64), -1)
    mask = torch.ones(2, 5, dtype=torch.bool)
    mask[1] = False
    s = s * mask.unsqueeze(-1)
    assert float(just_balance_loss(s, mask, batch_reduction="sum")) == float("-inf")
    assert float(R.dense_terms(s, mask).sum()) == float("-inf")


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from tgp import _native
    lib = _native.lib()
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)

    def terms(S=p, B=2, N=8, K=4, sizes=None, mask=None, ptr=None, max_rows=8, part=None, out=p, coef=p, mean=None):
        return lib.tgp_jb_terms_f32(S, B, N, K, sizes, mask, ptr, max_rows, 1, 8.0, 4.0, 1e-8, 1.0, part, out, coef, mean,
                                    None)
    assert terms(K=0) == -1 and b"tgp_jb_terms_f32" in lib.tgp_last_error()
    assert terms(B=-1) == -1 and terms(N=-1) == -1
    assert terms(S=None) == -1 and terms(out=None) == -1  # (coef and mean are optional outputs)
    assert b"null pointer" in lib.tgp_last_error()
    assert terms(ptr=p, mask=p, N=0) == -1 and terms(ptr=p, sizes=p, N=0) == -1  # an un-padded batch has neither
    assert terms(max_rows=9) == -1  # a padded batch has max_rows = N
    assert terms(N=100, max_rows=100) == -1 and b"part buffer" in lib.tgp_last_error()  # two splits, no part
    assert terms(N=1 << 31, max_rows=1 << 31, part=p) == -4
    assert terms(K=1 << 31) == -4 and terms(B=1 << 31) == -4
    assert terms(B=1 << 20, N=1 << 20, max_rows=1 << 20, part=p) == -4  # B x splits beyond int
    assert terms(N=1 << 24, max_rows=1 << 24, mask=p, part=p) == -4  # the mask count is exact below 2^24
    assert terms(sizes=p + 4) == -1 and b"misaligned" in lib.tgp_last_error()
    assert terms(ptr=p + 4, N=0, max_rows=8) == -1 and terms(out=p + 2) == -1 and terms(S=p + 1) == -1 and terms(mean=p + 2) == -1
    assert terms(B=0, S=None, out=None, coef=None) == 0  # nothing to do

    def ds(S=p, coef=p, g=p, rows=16, N=8, batch=None, B=2, K=4, out=p):
        return lib.tgp_jb_ds_f32(S, coef, g, 0, rows, N, batch, B, K, out, None)
    assert ds(K=0) == -1 and b"tgp_jb_ds_f32" in lib.tgp_last_error()
    assert ds(rows=-1) == -1 and ds(N=0) == -1
    assert ds(S=None) == -1 and ds(coef=None) == -1 and ds(g=None) == -1 and ds(out=None) == -1
    assert ds(K=1 << 31) == -4 and ds(N=1 << 31) == -4 and ds(rows=1 << 40) == -4
    assert ds(batch=p + 4) == -1 and ds(out=p + 2) == -1
    assert ds(rows=0, S=None, out=None) == 0
    assert lib.tgp_version() == 10044  # (appended entry points: the ABI number did not move)


def test_float32_host_tensors_do_not_reach_the_kernels():
    """The wrappers refuse host tensors (the composed form is what the loss functions take for them)."""
    from tgp import _native, kernels as K
    s = torch.softmax(torch.randn(2, 5, 3), -1)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        K.jb_terms(s)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        K.jb_ds(s, torch.zeros(2, 3), torch.ones(2))
