"""Edge-contraction pooling's public surface on the CPU: the reference's names, signatures and defaults
(poolers/edge_contraction.py:89-102, select/edge_contraction_select.py:150-157), ``repr``, exports, the alias set, the
state-dict names of the stored fixtures, the C ABI of the new entries, and that host tensors are refused (no CPU
fallback)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = torch.load(os.path.join(HERE, "golden", "golden_edgepool_v1.pt"), weights_only=True)["cases"]
NEW_SYMBOLS = ["tgp_edge_contract_max_graph_nodes", "tgp_edge_contract_edge_cache", "tgp_edge_contract_hub_degree",
               "tgp_edge_contract_workspace_bytes", "tgp_edge_contract_project_f32", "tgp_edge_contract_raw_f32",
               "tgp_edge_contract_normalize_f32", "tgp_edge_contract_graphs", "tgp_edge_contract_rounds_start",
               "tgp_edge_contract_rounds", "tgp_edge_contract_weights_f32"]


def test_constructors_match_the_reference():
    from tgp.poolers import EdgeContractionPooling
    from tgp.select import EdgeContractionSelect
    want = [("in_channels", inspect.Parameter.empty), ("edge_score_method", None), ("dropout", 0.0),
            ("add_to_edge_score", 0.5), ("lift", "precomputed"), ("s_inv_op", "transpose"), ("connect_red_op", "sum"),
            ("lift_red_op", "sum"), ("remove_self_loops", True), ("degree_norm", False), ("edge_weight_norm", False)]
    got = [(n, p.default) for n, p in inspect.signature(EdgeContractionPooling.__init__).parameters.items() if n != "self"]
    assert got == want
    want = [("in_channels", inspect.Parameter.empty), ("edge_score_method", None), ("dropout", 0.0),
            ("add_to_edge_score", 0.5), ("s_inv_op", "transpose")]
    got = [(n, p.default) for n, p in inspect.signature(EdgeContractionSelect.__init__).parameters.items() if n != "self"]
    assert got == want
    fwd = list(inspect.signature(EdgeContractionPooling.forward).parameters)
    assert fwd == ["self", "x", "adj", "edge_weight", "so", "batch", "lifting", "kwargs"]
    for name in ("softmax", "tanh", "sigmoid"):
        fn = getattr(EdgeContractionSelect, "compute_edge_score_" + name)
        assert list(inspect.signature(fn).parameters) == ["raw_edge_score", "edge_index", "num_nodes"]
        assert isinstance(inspect.getattr_static(EdgeContractionSelect, "compute_edge_score_" + name), staticmethod)


def test_repr_is_the_reference_one():
    from tgp.poolers import EdgeContractionPooling
    from tgp.select import EdgeContractionSelect
    assert repr(EdgeContractionSelect(in_channels=4)) == (
        "EdgeContractionSelect(in_channels=4, edge_score_method=compute_edge_score_softmax, dropout=0.0, "
        "add_to_edge_score=0.5, s_inv_op=transpose)")
    sel = EdgeContractionSelect(7, EdgeContractionSelect.compute_edge_score_tanh, dropout=0.2, add_to_edge_score=0.0,
                                s_inv_op="inverse")
    assert repr(sel) == ("EdgeContractionSelect(in_channels=7, edge_score_method=compute_edge_score_tanh, dropout=0.2, "
                         "add_to_edge_score=0.0, s_inv_op=inverse)")

    def my_score(raw, edge_index, num_nodes):
        return raw

    assert "edge_score_method=my_score" in repr(EdgeContractionSelect(3, my_score))
    p = EdgeContractionPooling(in_channels=4, connect_red_op="max")
    assert "EdgeContractionSelect(in_channels=4" in repr(p) and "SparseConnect(reduce_op=max" in repr(p)


def test_state_dict_names_and_shapes():
    from tgp.poolers import EdgeContractionPooling
    from tgp.select import EdgeContractionSelect
    for name, c in CASES.items():
        method = getattr(EdgeContractionSelect, "compute_edge_score_" + c["method"])
        p = EdgeContractionPooling(edge_score_method=method, **c["cfg"])
        assert sorted(p.state_dict()) == sorted(c["params"]), name
        p.load_state_dict(c["params"])
    p = EdgeContractionPooling(in_channels=5)
    assert sorted(p.state_dict()) == ["selector.lin.bias", "selector.lin.weight"]
    assert p.state_dict()["selector.lin.weight"].shape == (1, 10) and p.state_dict()["selector.lin.bias"].shape == (1,)
    assert isinstance(p.selector.lin, torch.nn.Linear)


def test_exports_and_alias_set():
    import tgp.poolers as P
    import tgp.select as S
    assert "EdgeContractionPooling" in P.pooler_classes and "EdgeContractionPooling" in P.__all__
    assert P.pooler_classes == sorted(P.pooler_classes)
    # the alias set is pinned to the five poolers of the hot path
    assert sorted(P.pooler_map) == ["diff", "graclus", "mincut", "ndp", "topk"]
    assert "edgepool" not in P.pooler_map
    with pytest.raises(ValueError, match="Unknown pooler_name"):
        P.get_pooler("edgepool", in_channels=4)
    for name in ("EdgeContractionSelect", "maximal_matching", "maximal_matching_cluster"):
        assert name in S.__all__ and hasattr(S, name), name
    for fn in (S.maximal_matching, S.maximal_matching_cluster):
        assert [(n, p.default) for n, p in inspect.signature(fn).parameters.items()] == [
            ("edge_index", inspect.Parameter.empty), ("num_nodes", None), ("perm", None)]


def test_host_tensors_have_no_cpu_fallback():
    from tgp import _native, kernels
    from tgp.poolers import EdgeContractionPooling
    from tgp.select import EdgeContractionSelect, maximal_matching, maximal_matching_cluster
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    x = torch.randn(3, 4)
    for method in (None, EdgeContractionSelect.compute_edge_score_tanh, lambda r, e, n: r):
        with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
            EdgeContractionPooling(in_channels=4, edge_score_method=method)(x=x, adj=ei)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        EdgeContractionSelect(4)(x, ei)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        maximal_matching(ei, 3)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        maximal_matching_cluster(ei, 3, torch.tensor([3, 1, 0, 2]))
    for fn in (EdgeContractionSelect.compute_edge_score_softmax, EdgeContractionSelect.compute_edge_score_tanh,
               EdgeContractionSelect.compute_edge_score_sigmoid):
        with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
            fn(torch.randn(4), ei, 3)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        kernels.edge_contract_scores(x, ei, torch.randn(8), torch.randn(1))
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        kernels.edge_contract_select(ei, 3, torch.rand(4))


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from tgp import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tgp_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tgp_edge_contract_[a-z0-9_]+)\s*\(", text))
    assert declared == set(NEW_SYMBOLS)
    assert {s for s in _native.SIGNATURES if s.startswith("tgp_edge_contract_")} == set(NEW_SYMBOLS)
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name
    lib = _native.lib()
    assert lib.tgp_version() == 10044
    assert lib.tgp_edge_contract_max_graph_nodes() == 1024
    assert lib.tgp_edge_contract_edge_cache() == 4096
    assert lib.tgp_edge_contract_hub_degree() == 512
    assert lib.tgp_edge_contract_workspace_bytes(1000) >= 1000 * (2 * 8 + 1)


def test_new_entry_points_validate_without_a_gpu():
    from tgp import _native
    lib = _native.lib()
    d = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(d)
    big = 1 << 32
    assert lib.tgp_edge_contract_project_f32(p, 4, 8, 4, p, p, None) == -1  # row stride below F
    assert b"tgp_edge_contract_project_f32" in lib.tgp_last_error()
    assert lib.tgp_edge_contract_project_f32(None, 4, 8, 8, p, p, None) == -1
    assert lib.tgp_edge_contract_raw_f32(p, p, big, 4, p, None, p, None) == -4  # E >= 2^32
    assert lib.tgp_edge_contract_raw_f32(None, p, 4, 4, p, None, p, None) == -1
    assert lib.tgp_edge_contract_normalize_f32(p, p, 4, 4, 3, 0.5, p, p, p, p, 4, p + 8, None) == -1  # unknown method
    assert lib.tgp_edge_contract_normalize_f32(p, p, 4, 4, 1, 0.5, None, None, None, None, 0, p, None) == -1  # raw == out
    assert lib.tgp_edge_contract_normalize_f32(p, p, 4, 4, 0, 0.5, None, None, p, p, 4, p + 8, None) == -1  # no index
    assert lib.tgp_edge_contract_normalize_f32(p, p, 4096, 4, 0, 0.5, p, p, p, p, 1, p + 8, None) == -2  # hub queue
    assert lib.tgp_edge_contract_graphs(p, p, 4, 4, p, 1, 2048, p, None, p, p, p, p, None) == -4  # graph too long
    assert b"tgp_edge_contract_graphs" in lib.tgp_last_error()
    assert lib.tgp_edge_contract_graphs(p, p, big, 4, p, 1, 64, p, None, p, p, p, p, None) == -4
    assert lib.tgp_edge_contract_graphs(p, p, 4, 4, p, 1, 64, None, None, p, p, p, p, None) == -1  # no priorities
    assert lib.tgp_edge_contract_rounds_start(100, 4, p, 8, p, p, p, None) == -2
    assert b"workspace too small" in lib.tgp_last_error()
    assert lib.tgp_edge_contract_rounds_start(100, big, p, 1 << 20, p, p, p, None) == -4
    assert lib.tgp_edge_contract_rounds(p, p, 4, 4, p, None, p, 0, 1, None, p, p, p, None) == -1  # no flags
    assert lib.tgp_edge_contract_rounds(p, p, big, 4, p, None, p, 0, 1, p, p, p, p, None) == -4
    assert lib.tgp_edge_contract_weights_f32(None, p, 4, 4, p, None) == -1


def test_bad_arguments_to_the_host_entries():
    """Checks that run before any device work (the device check comes first, so these need device-free failures)."""
    from tgp import kernels
    assert kernels.EC_METHODS == {"softmax": 0, "tanh": 1, "sigmoid": 2}
    sig = inspect.signature(kernels.edge_contract_select)
    assert list(sig.parameters)[:6] == ["edge_index", "num_nodes", "score", "graph_ptr", "max_graph_nodes", "route"]
    assert kernels.EdgeContractResult.__slots__[:2] == ("index", "k")
    for field in ("index", "k", "match", "weight", "route", "rounds"):
        assert hasattr(kernels.EdgeContractResult, field), field
