"""AsymCheegerCut pooling's public surface on the CPU: the reference's names, signatures and defaults
(poolers/asym_cheeger_cut.py:97-136, utils/losses.py:503-550, 780-1010), the module's state-dict names, the float64 loss
functions against the reference's float64 values (tests/golden/golden_acc_v1.pt) at 1e-12, and the argument checks of
the new entry points, which answer before any launch."""
import ctypes
import inspect
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_acc_v1.pt"), weights_only=True)["cases"]


def test_constructor_matches_the_reference():
    from tgp.poolers import AsymCheegerCutPooling
    sig = inspect.signature(AsymCheegerCutPooling.__init__)
    want = [("in_channels", inspect.Parameter.empty), ("k", inspect.Parameter.empty), ("act", None), ("dropout", 0.0),
            ("totvar_coeff", 1.0), ("balance_coeff", 1.0), ("remove_self_loops", True), ("degree_norm", True),
            ("edge_weight_norm", False), ("adj_transpose", True), ("lift", "precomputed"), ("s_inv_op", "transpose"),
            ("batched", True), ("sparse_output", False), ("cache_preprocessing", False)]
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self"]
    assert got == want
    names = [n for n, _ in want]
    for c in CASES.values():  # every stored cfg is a call of that signature
        if c["kind"] == "pool":
            assert set(c["cfg"]) <= set(names)


def test_exports_and_alias_set():
    import tgp.poolers as P
    assert "AsymCheegerCutPooling" in P.pooler_classes and "AsymCheegerCutPooling" in P.__all__
    assert "acc" not in P.pooler_map  # the alias is a follow-up (the alias set is pinned to five poolers)
    assert P.AsymCheegerCutPooling._loss_kind == "acc"
    from tgp.utils import losses
    for name, params in (
        ("totvar_loss", ["S", "adj", "batch_reduction"]),
        ("sparse_totvar_loss", ["edge_index", "S", "edge_weight", "batch", "batch_reduction"]),
        ("asym_norm_loss", ["S", "k", "mask", "batch_reduction"]),
        ("unbatched_asym_norm_loss", ["S", "k", "batch", "batch_reduction"]),
    ):
        sig = inspect.signature(getattr(losses, name))
        assert list(sig.parameters) == params, name
        assert sig.parameters["batch_reduction"].default == "mean", name


def test_state_dict_names_and_repr_args():
    from tgp.poolers import AsymCheegerCutPooling
    for name in ("acc_batched_default_w", "acc_batched_mlp2_w", "acc_u_single_graph"):
        c = CASES[name]
        p = AsymCheegerCutPooling(**c["cfg"], batched=c["alias"] == "acc")
        assert sorted(p.state_dict()) == sorted(c["params"]), name
        assert all(k.startswith("selector.mlp.lins.") for k in p.state_dict())
        p.load_state_dict(c["params"])
    p = AsymCheegerCutPooling(in_channels=5, k=4, balance_coeff=0.5, batched=False)
    assert p.extra_repr_args() == {"batched": False, "totvar_coeff": 1.0, "balance_coeff": 0.5}


def test_loss_only_kinds_share_one_predicate():
    from tgp.poolers import AsymCheegerCutPooling, DiffPool, DMoNPooling, MinCutPooling
    want = {DiffPool: (False, False), MinCutPooling: (False, True), DMoNPooling: (True, True),
            AsymCheegerCutPooling: (True, False)}
    for cls, (loss_only, wants_raw) in want.items():
        p = cls(in_channels=4, k=3)
        assert (p._loss_only, p._wants_raw) == (loss_only, wants_raw), cls.__name__


def test_float64_loss_forms_match_the_reference():
    import sys
    sys.path.insert(0, HERE)
    from test_acc_restatement import Package, function_values
    c = CASES["acc_functions_f64"]
    i, e = c["inputs"], c["expected"]
    got = function_values(Package, i, int(i["batch"].max()) + 1)
    from tgp.utils.losses import asym_norm_loss, totvar_loss
    got["totvar_sum"] = totvar_loss(i["s"], i["adj"], batch_reduction="sum")
    got["asym_sum"] = asym_norm_loss(i["s"], i["s"].size(-1), mask=i["mask"], batch_reduction="sum")
    assert set(got) == set(e)
    for k, v in got.items():
        assert v.dtype == torch.float64, k
        scale = max(abs(float(e[k])), 1.0) if "asym" in k else abs(float(e[k]))
        assert abs(float(v) - float(e[k])) <= 1e-12 * scale, (k, float(v), float(e[k]))


def test_float32_host_tensors_have_no_cpu_fallback():
    from tgp import _native
    from tgp.utils.losses import asym_norm_loss, sparse_totvar_loss, totvar_loss, unbatched_asym_norm_loss
    s = torch.softmax(torch.randn(2, 5, 3), -1)
    a = (torch.rand(2, 5, 5) < 0.5).float()
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    batch = torch.zeros(5, dtype=torch.long)
    for call in (lambda: totvar_loss(s, a), lambda: asym_norm_loss(s, 3), lambda: asym_norm_loss(s, 3, mask=a[:, 0] > 0),
                 lambda: sparse_totvar_loss(ei, s[0]), lambda: sparse_totvar_loss(ei, s[0], torch.ones(3), batch),
                 lambda: unbatched_asym_norm_loss(s[0], 3), lambda: unbatched_asym_norm_loss(s[0], 3, batch)):
        with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
            call()


def test_new_entry_points_validate_without_a_gpu():
    from tgp import _native
    lib = _native.lib()
    assert lib.tgp_version() == 10044  # (appended entry points: the ABI number did not move)
    assert lib.tgp_acc_small_graph_nodes() == 128
    d = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(d)
    INVALID, RANGE = -1, -4
    # dense total variation: nrb must be ceil(N / 16); null outputs; sizes beyond the int32 indices
    assert lib.tgp_acc_tv_dense_f32(p, p, 1, 32, 4, None, 1, p, p, None) == INVALID
    assert b"tgp_acc_tv_dense_f32" in lib.tgp_last_error()
    assert lib.tgp_acc_tv_dense_f32(p, p, 1, 32, 4, None, 2, None, p, None) == INVALID
    assert lib.tgp_acc_tv_dense_f32(p, p, 1, 32, 0, None, 2, p, p, None) == INVALID
    assert lib.tgp_acc_tv_dense_f32(p, p, 70000, 32, 4, None, 2, p, p, None) == RANGE
    assert lib.tgp_acc_tv_dense_f32(p, p, 0, 32, 4, None, 2, None, None, None) == 0  # (an empty batch launches nothing)
    assert lib.tgp_acc_tv_dense_bwd_f32(p, p, 1, 32, 4, None, None, p, 1.0, p, None) == INVALID
    assert b"tgp_acc_tv_dense_bwd_f32" in lib.tgp_last_error()
    assert lib.tgp_acc_tv_dense_bwd_f32(p, p, 1, -1, 4, None, p, p, 1.0, p, None) == INVALID
    assert lib.tgp_acc_tv_dense_bwd_f32(p, p, 1, 32, 40000, None, p, p, 1.0, p, None) == RANGE
    # edge total variation
    assert lib.tgp_acc_tv_edge_f32(p, 4, 2, None, None, 3, p, p, p, None) == INVALID  # edges without destinations
    assert b"tgp_acc_tv_edge_f32" in lib.tgp_last_error()
    assert lib.tgp_acc_tv_edge_f32(p, 4, 2, p, None, 3, None, p, p, None) == INVALID
    assert lib.tgp_acc_tv_edge_f32(p, 1 << 31, 2, p, None, 3, p, p, p, None) == RANGE
    assert lib.tgp_acc_tv_edge_f32(p, 0, 2, None, None, 0, None, None, None, None) == 0
    assert lib.tgp_acc_tv_edge_bwd_f32(p, 4, 2, p, p, None, 3, p, p, None, p, None, p, p, 1.0, 1, p, None) == INVALID
    assert b"tgp_acc_tv_edge_bwd_f32" in lib.tgp_last_error()
    assert lib.tgp_acc_tv_edge_bwd_f32(p, 4, 2, p, p, None, 3, p, p, p, p, None, p, p, 1.0, 0, p, None) == INVALID  # B = 0
    # quantile select
    assert lib.tgp_acc_quantile_f32(p, 1, 200, 4, None, None, None, 200, 4, 1, p, p, p, p, p, None) == RANGE
    assert b"at most 128 nodes" in lib.tgp_last_error()
    assert lib.tgp_acc_quantile_f32(p, 1, 64, 4, None, None, None, 64, 4, 3, p, p, p, p, p, None) == INVALID  # route
    assert lib.tgp_acc_quantile_f32(p, 1, 64, 4, p, None, p, 64, 4, 0, p, p, p, p, p, None) == INVALID  # sizes + ptr
    assert lib.tgp_acc_quantile_f32(p, 1, 64, 4, None, None, None, 32, 4, 0, p, p, p, p, p, None) == INVALID  # max_nodes != N
    assert lib.tgp_acc_quantile_f32(p, 1, 64, 4, None, None, None, 64, 4, 0, p, None, p, p, p, None) == INVALID
    assert lib.tgp_acc_quantile_f32(p, 1, 64, 40000, None, None, None, 64, 4, 0, p, p, p, p, p, None) == RANGE
    # tail
    assert lib.tgp_acc_loss_terms_f32(p, None, None, None, 2, None, None, 1, 4, 4, 1.0, 1.0, p, p, None) == INVALID
    assert b"tgp_acc_loss_terms_f32" in lib.tgp_last_error()
    assert lib.tgp_acc_loss_terms_f32(p, None, p, None, 0, None, None, 1, 4, 4, 1.0, 1.0, p, p, None) == INVALID  # no ptr
    assert lib.tgp_acc_loss_terms_f32(None, None, None, None, 0, p, None, 1, 4, 4, 1.0, 1.0, p, p, None) == INVALID
    assert lib.tgp_acc_loss_terms_f32(None, None, None, None, 0, None, None, 1, 4, 4, 1.0, 1.0, None, p, None) == INVALID
    # balance backward
    assert lib.tgp_acc_asym_bwd_f32(p, 4, 0, 2, None, None, None, None, p, p, p, p, p, 1.0, 2, 1, 0, p, None) == INVALID
    assert b"tgp_acc_asym_bwd_f32" in lib.tgp_last_error()
    assert lib.tgp_acc_asym_bwd_f32(p, 4, 0, 2, None, p, None, p, p, p, p, p, p, 1.0, 2, 1, 0, p, None) == INVALID
    assert lib.tgp_acc_asym_bwd_f32(p, 4, 4, 2, None, None, None, None, None, p, p, p, p, 1.0, 2, 1, 0, p, None) == INVALID
    assert lib.tgp_acc_asym_bwd_f32(p, 1 << 41, 4, 2, None, None, None, None, p, p, p, p, p, 1.0, 2, 1, 0, p, None) == RANGE
