"""k-MIS pooling's public surface on the CPU: the reference's names, signatures and defaults (poolers/kmis.py:128-144,
select/kmis_select.py:232-243), exports, the alias set, the state-dict names of the stored fixtures, the caching
exception, and that host tensors are refused (no CPU fallback)."""
import inspect
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_kmis_v1.pt"), weights_only=True)["cases"]


def test_constructors_match_the_reference():
    from tgp.poolers import KMISPooling
    from tgp.select import KMISSelect
    want = [("in_channels", None), ("order_k", 1), ("scorer", "linear"), ("score_heuristic", "greedy"),
            ("force_undirected", False), ("lift", "precomputed"), ("s_inv_op", "transpose"), ("reduce_red_op", "sum"),
            ("connect_red_op", "sum"), ("lift_red_op", "sum"), ("remove_self_loops", True), ("degree_norm", False),
            ("edge_weight_norm", False), ("cached", False)]
    got = [(n, p.default) for n, p in inspect.signature(KMISPooling.__init__).parameters.items() if n != "self"]
    assert got == want
    want = [("in_channels", None), ("order_k", 1), ("scorer", "linear"), ("score_heuristic", "greedy"),
            ("force_undirected", False), ("s_inv_op", "transpose")]
    got = [(n, p.default) for n, p in inspect.signature(KMISSelect.__init__).parameters.items() if n != "self"]
    assert got == want
    assert KMISSelect._heuristics == {None, "greedy", "w-greedy"}
    assert KMISSelect._scorers == {"linear", "degree", "random", "constant", "canonical"}


def test_exports_and_alias_set():
    import tgp.poolers as P
    import tgp.select as S
    assert "KMISPooling" in P.pooler_classes and "KMISPooling" in P.__all__
    assert "kmis" not in P.pooler_map  # the alias is a follow-up (the alias set is pinned to five poolers)
    for name in ("KMISSelect", "maximal_independent_set", "maximal_independent_set_cluster", "degree_scorer"):
        assert name in S.__all__ and hasattr(S, name), name
    for fn in (S.maximal_independent_set, S.maximal_independent_set_cluster):
        sig = inspect.signature(fn)
        assert [(n, p.default) for n, p in sig.parameters.items()] == [
            ("edge_index", inspect.Parameter.empty), ("order_k", 1), ("perm", None), ("num_nodes", None)]
    assert list(inspect.signature(S.degree_scorer).parameters) == ["edge_index", "edge_weight", "num_nodes", "dim"]


def test_state_dict_names_repr_and_flags():
    from tgp.poolers import KMISPooling
    from tgp.select import KMISSelect
    for name, c in CASES.items():
        p = KMISPooling(**c["cfg"])
        assert sorted(p.state_dict()) == sorted(c["params"]), name
        p.load_state_dict(c["params"])
        assert p.precoarsenable == (c["cfg"].get("scorer", "linear") != "linear")
    p = KMISPooling(in_channels=4, order_k=2)
    assert sorted(p.state_dict()) == ["selector.lin.bias", "selector.lin.weight"]
    assert p.state_dict()["selector.lin.weight"].shape == (1, 4) and p.state_dict()["selector.lin.bias"].shape == (1,)
    assert p.extra_repr_args() == {"cached": False}
    assert repr(KMISSelect(in_channels=[4, 3], order_k=2)) == (
        "KMISSelect(order_k=2, scorer=linear, score_heuristic=greedy, force_undirected=False, s_inv_op=transpose)")


def test_rejected_configurations():
    from tgp.poolers import KMISPooling
    from tgp.select import KMISSelect
    with pytest.raises(Exception, match="Caching should be disabled"):
        KMISPooling(in_channels=4, cached=True)
    KMISPooling(scorer="degree", cached=True)
    for bad in ("first", "last", lambda x: x):
        with pytest.raises(AssertionError, match="Unrecognized `scorer`"):
            KMISSelect(scorer=bad)
    with pytest.raises(AssertionError, match="Unrecognized `score_heuristic`"):
        KMISSelect(in_channels=4, score_heuristic="best")
    with pytest.raises(ValueError, match="canonical"):
        KMISSelect(scorer="canonical", score_heuristic="w-greedy")
    KMISSelect(scorer="canonical", score_heuristic=None)


def test_host_tensors_have_no_cpu_fallback():
    from tgp import _native
    from tgp.poolers import KMISPooling
    from tgp.select import degree_scorer, maximal_independent_set, maximal_independent_set_cluster
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    x = torch.randn(3, 4)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        KMISPooling(in_channels=4)(x=x, adj=ei)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        KMISPooling(scorer="degree")(x=x, adj=ei, edge_weight=torch.rand(4))
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        maximal_independent_set(ei, 1)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        maximal_independent_set_cluster(ei, 2, torch.tensor([2, 0, 1]))
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        degree_scorer(ei, torch.rand(4), 3)


def test_new_entry_points_validate_without_a_gpu():
    import ctypes
    from tgp import _native
    lib = _native.lib()
    assert lib.tgp_version() == 10044
    assert lib.tgp_kmis_max_graph_nodes() == 1024
    assert lib.tgp_kmis_workspace_bytes(1000) >= 1000 * (4 * 8 + 4)
    d = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(d)
    assert lib.tgp_kmis_graphs(p, p, 4, 4, p, 1, 2048, 1, 0, None, p, None, p, p, None) == -4  # graph too long
    assert b"tgp_kmis_graphs" in lib.tgp_last_error()
    assert lib.tgp_kmis_graphs(p, p, 4, 4, p, 1, 64, 1, 2, p, None, None, p, p, None) == -1  # "greedy" without its output
    assert lib.tgp_kmis_rounds_start(p, None, 100, p, 8, None) == -2
    assert b"workspace too small" in lib.tgp_last_error()
    assert lib.tgp_kmis_rounds(p, p, 4, 4, 0, p, 0, 1, p, None) == -1  # order_k = 0
    assert lib.tgp_kmis_clusters(p, p, 4, 4, 1, None, 0, p, None) == -1
    assert lib.tgp_kmis_greedy_f32(p, p, 4, 100, 1, p, p, 8, p, None) == -2
    assert lib.tgp_kmis_wsum_f32(p, None, None, p, None, 4, p, None) == -1
    assert lib.tgp_kmis_degree_f32(None, None, None, 4, p, None) == -1
    assert lib.tgp_kmis_mis_index_i64(None, p, 4, p, None) == -1
