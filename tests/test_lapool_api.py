"""LaPool's public surface on the CPU: the reference's names, signatures and defaults (poolers/lapool.py:78-89,
select/lapool_select.py:125-130), ``repr``, exports, the alias set, the input checks and their messages, the C ABI of the
new entries, and that host tensors are refused (no CPU fallback)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ["tgp_lapool_variation_dense_f32", "tgp_lapool_variation_csr_f32", "tgp_lapool_flags_dense_f32",
               "tgp_lapool_flags_csr_f32", "tgp_lapool_columns", "tgp_lapool_assign_f32", "tgp_lapool_assign_bwd_f32"]


def test_constructors_match_the_reference():
    from tgp.poolers import LaPooling
    from tgp.select import LaPoolSelect
    want = [("shortest_path_reg", False), ("remove_self_loops", True), ("degree_norm", True), ("edge_weight_norm", False),
            ("lift", "precomputed"), ("s_inv_op", "transpose"), ("lift_red_op", "sum"), ("batched", True),
            ("sparse_output", False)]
    got = [(n, p.default) for n, p in inspect.signature(LaPooling.__init__).parameters.items() if n != "self"]
    assert got == want
    want = [("shortest_path_reg", False), ("batched_representation", True), ("s_inv_op", "transpose")]
    got = [(n, p.default) for n, p in inspect.signature(LaPoolSelect.__init__).parameters.items() if n != "self"]
    assert got == want
    fwd = list(inspect.signature(LaPooling.forward).parameters)
    assert fwd == ["self", "x", "adj", "edge_weight", "so", "batch", "batch_pooled", "lifting", "mask", "kwargs"]
    fwd = list(inspect.signature(LaPoolSelect.forward).parameters)
    assert fwd == ["self", "x", "edge_index", "edge_weight", "batch", "mask", "num_nodes", "kwargs"]
    assert LaPoolSelect.is_dense is True


def test_repr_and_parts():
    from tgp.connect import DenseConnect
    from tgp.lift import BaseLift
    from tgp.poolers import LaPooling
    from tgp.reduce import BaseReduce
    from tgp.select import LaPoolSelect
    assert repr(LaPoolSelect(s_inv_op="inverse")) == "LaPoolSelect(s_inv_op=inverse, shortest_path_reg=False)"
    p = LaPooling(batched=False, degree_norm=False, sparse_output=True, lift="transpose", lift_red_op="mean")
    assert p.extra_repr_args() == {"batched": False}
    assert "batched=False" in repr(p) and "LaPoolSelect(s_inv_op=transpose" in repr(p)
    assert type(p.selector) is LaPoolSelect and type(p.reducer) is BaseReduce
    assert type(p.connector) is DenseConnect and type(p.lifter) is BaseLift
    assert p.connector.degree_norm is False and p.connector.sparse_output is True and p.connector.remove_self_loops is True
    assert p.lifter.matrix_op == "transpose" and p.lifter.reduce_op == "mean"
    assert p.selector.batched_representation is False and p.batched is False and p.sparse_output is True
    assert list(p.state_dict()) == []  # no learned layer


def test_exports_and_alias_set():
    import tgp.poolers as P
    import tgp.select as S
    assert "LaPooling" in P.pooler_classes and "LaPooling" in P.__all__
    assert P.pooler_classes == sorted(P.pooler_classes)
    assert sorted(P.pooler_map) == ["diff", "graclus", "mincut", "ndp", "topk"]  # still the five of the hot path
    assert "lap" not in P.pooler_map
    with pytest.raises(ValueError, match="Unknown pooler_name"):
        P.get_pooler("lap")
    assert "LaPoolSelect" in S.__all__ and hasattr(S, "LaPoolSelect")


def test_shortest_path_reg_is_not_built():
    from tgp.poolers import LaPooling
    from tgp.select import LaPoolSelect
    with pytest.raises(NotImplementedError, match="shortest_path_reg"):
        LaPoolSelect(shortest_path_reg=True)
    with pytest.raises(NotImplementedError, match="shortest_path_reg"):
        LaPooling(shortest_path_reg=True)


def test_input_checks_carry_the_reference_messages():
    from tgp.select import LaPoolSelect
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    x, adj = torch.randn(3, 4), torch.rand(3, 3)
    b, u = LaPoolSelect(), LaPoolSelect(batched_representation=False)
    with pytest.raises(ValueError, match=re.escape("x must have shape [B, N, F].")):
        b(torch.randn(2, 2, 3, 4), adj)
    with pytest.raises(ValueError, match="Batched LaPoolSelect expects a dense adjacency tensor."):
        b(x, ei)
    with pytest.raises(ValueError, match="Batched LaPoolSelect expects a dense adjacency tensor."):
        b(x, torch.rand(1, 1, 3, 3))  # (4-D is no dense adjacency to is_dense_adj, here as in the reference)
    with pytest.raises(ValueError, match=re.escape("x must have shape [N, F].")):
        u(x.unsqueeze(0), ei)
    with pytest.raises(ValueError, match="mask is only supported for batched representations."):
        u(x, ei, mask=torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError, match="Unbatched LaPoolSelect expects a sparse adjacency tensor."):
        u(x, adj)


def test_host_tensors_have_no_cpu_fallback():
    from tgp import _native, kernels
    from tgp.poolers import LaPooling
    from tgp.select import LaPoolSelect
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    x, adj = torch.randn(3, 4), torch.rand(1, 3, 3)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        LaPoolSelect()(x, adj)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        LaPoolSelect(batched_representation=False)(x, ei)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        LaPooling(batched=False)(x=x, adj=ei)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        kernels.lapool_variation(x.unsqueeze(0), adj)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        kernels.lapool_variation(x, edge_index=ei)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        kernels.lapool_leaders(torch.rand(1, 3), adj)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        kernels.lapool_columns(torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError, match="either a padded adjacency or an edge list"):
        kernels.lapool_variation(x)
    for name in ("lapool_variation", "lapool_leaders", "lapool_columns", "lapool_assign", "lapool_assign_bwd"):
        assert callable(getattr(kernels, name)), name


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from tgp import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tgp_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tgp_lapool_[a-z0-9_]+)\s*\(", text))
    assert declared == set(NEW_SYMBOLS)
    assert {s for s in _native.SIGNATURES if s.startswith("tgp_lapool_")} == set(NEW_SYMBOLS)
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name
    assert _native.lib().tgp_version() == 10044


def test_new_entry_points_validate_without_a_gpu():
    from tgp import _native
    lib = _native.lib()
    d = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(d)
    big = 1 << 31
    assert lib.tgp_lapool_variation_dense_f32(p, p, 2, 3, 4, None, None, None) == -1  # no output
    assert b"tgp_lapool_variation_dense_f32" in lib.tgp_last_error()
    assert lib.tgp_lapool_variation_dense_f32(None, p, 2, 3, 4, None, p, None) == -1
    assert lib.tgp_lapool_variation_dense_f32(p, p, 1 << 20, 1 << 20, 4, None, p, None) == -4  # B N beyond int32
    assert lib.tgp_lapool_variation_dense_f32(p, p, 2, 3, big, None, p, None) == -4
    assert lib.tgp_lapool_variation_csr_f32(p, None, p, None, p, 3, 4, 4, None, None) == -1
    assert lib.tgp_lapool_variation_csr_f32(None, None, p, None, p, 3, 4, 4, p, None) == -1
    assert lib.tgp_lapool_variation_csr_f32(p, None, p, None, p, 3, big, 4, p, None) == -4
    assert lib.tgp_lapool_variation_csr_f32(p, None, p, None, p, big, 4, 4, p, None) == -4
    assert lib.tgp_lapool_flags_dense_f32(p, p, 2, 3, None, None, None) == -1
    assert lib.tgp_lapool_flags_dense_f32(p, None, 2, 3, None, p, None) == -1
    assert lib.tgp_lapool_flags_dense_f32(p, p, 1 << 20, 1 << 20, None, p, None) == -4
    assert lib.tgp_lapool_flags_csr_f32(p, None, p, p, 3, 4, None, None) == -1
    assert lib.tgp_lapool_flags_csr_f32(p, None, p, p, big, 4, p, None) == -4
    assert lib.tgp_lapool_columns(p, 6, 2, 3, None, None, 1, None, p, p, p, None) == -1  # no col_of
    assert lib.tgp_lapool_columns(p, 7, 2, 3, None, None, 1, p, p, p, p, None) == -1  # rows != B N
    assert b"padded batch" in lib.tgp_last_error()
    assert lib.tgp_lapool_columns(p, 6, 2, 0, p, p, 1, p, p, p, p, None) == -1  # a mask with offsets
    assert lib.tgp_lapool_columns(None, 6, 2, 3, None, None, 1, p, p, p, p, None) == -1  # no flags
    assert lib.tgp_lapool_columns(p, big, 1, big, None, None, 1, p, p, p, p, None) == -4
    assert lib.tgp_lapool_assign_f32(p, 6, 4, 2, 3, None, None, None, p, p, p, 2, 1e-8, None, p, None) == -1
    assert lib.tgp_lapool_assign_f32(p, 6, 4, 2, 0, None, p, None, p, p, p, 2, 1e-8, p, p, None) == -1  # no batch vector
    assert b"batch vector" in lib.tgp_last_error()
    assert lib.tgp_lapool_assign_f32(p, 6, 4, 2, 3, None, None, None, None, p, p, 2, 1e-8, p, p, None) == -1
    assert lib.tgp_lapool_assign_f32(p, 6, 4, 2, 3, None, None, None, p, p, p, big, 1e-8, p, p, None) == -4
    assert lib.tgp_lapool_assign_bwd_f32(p, p, p, p, 6, 4, 2, 3, None, None, None, p, p, p, 2, 1e-8, p, p, p, None,
                                         None) == -1  # no dX
    assert lib.tgp_lapool_assign_bwd_f32(p, p, p, p, 6, 4, 2, 3, None, None, None, p, p, p, 2, 1e-8, None, p, p, p,
                                         None) == -1  # no work buffer
    assert lib.tgp_lapool_assign_bwd_f32(p, p, p, p, 6, big, 2, 3, None, None, None, p, p, p, 2, 1e-8, p, p, p, p,
                                         None) == -4
