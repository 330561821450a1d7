"""HOSC's public surface on the CPU: the reference's names, signatures and defaults (poolers/hosc.py:104-122,
utils/losses.py:218-224, 392-396, 597-601), the module's state-dict names, and the float64 loss forms against the
reference's float64 values (tests/golden/golden_hosc_v1.pt) at 1e-12."""
import inspect
import math
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_hosc_v1.pt"), weights_only=True)["cases"]


def test_constructor_matches_the_reference():
    from tgp.poolers import HOSCPooling
    sig = inspect.signature(HOSCPooling.__init__)
    want = [("in_channels", inspect.Parameter.empty), ("k", inspect.Parameter.empty), ("act", None), ("dropout", 0.0),
            ("mu", 0.1), ("alpha", 0.5), ("hosc_ortho", False), ("remove_self_loops", True), ("degree_norm", True),
            ("edge_weight_norm", False), ("adj_transpose", True), ("lift", "precomputed"), ("s_inv_op", "transpose"),
            ("batched", True), ("sparse_output", False), ("cache_preprocessing", False)]
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self"]
    assert got == want


def test_exports_and_alias_set():
    import tgp.poolers as P
    assert "HOSCPooling" in P.pooler_classes and "HOSCPooling" in P.__all__
    assert "hosc" not in P.pooler_map  # the alias is a follow-up (the alias set is pinned to five poolers)
    assert "hosc" in P.__doc__
    assert P.HOSCPooling._loss_kind == "hosc"
    assert "hosc" in P._DenseMLPPooling._LOSS_ONLY_KINDS and "hosc" in P._DenseMLPPooling._DENSE_ADJ_LOSS_KINDS
    assert P.HOSCPooling(in_channels=3, k=2)._wants_raw
    from tgp.utils import losses
    for name, params, default in (
        ("hosc_orthogonality_loss", ["S", "mask", "batch_reduction"], [None, "mean"]),
        ("unbatched_hosc_orthogonality_loss", ["S", "batch", "batch_reduction"], [None, "mean"]),
        ("sparse_ho_mincut_loss", ["edge_index", "S", "edge_weight", "batch", "batch_reduction"], [None, None, "mean"]),
    ):
        sig = inspect.signature(getattr(losses, name))
        assert list(sig.parameters) == params, name
        assert [p.default for p in sig.parameters.values() if p.default is not p.empty] == default, name
    for name in ("hosc_loss_terms", "hosc_sparse_loss_terms", "_HOSCTermsFn"):
        assert hasattr(losses, name), name


def test_state_dict_names_and_repr_args():
    from tgp.poolers import HOSCPooling
    for name in ("hosc_default", "hosc_mlp2", "hosc_u_single_graph", "hosc_k1_hosc_ortho"):
        c = CASES[name]
        p = HOSCPooling(**c["cfg"], batched=c["alias"] == "hosc")
        assert sorted(p.state_dict()) == sorted(c["params"]), name
        p.load_state_dict(c["params"])
    p = HOSCPooling(in_channels=5, k=4, mu=0.3, alpha=0.25, hosc_ortho=True, batched=False)
    assert p.extra_repr_args() == {"batched": False, "mu": 0.3, "alpha": 0.25, "hosc_ortho": True}


def _function_values(i):
    from tgp.utils.losses import hosc_orthogonality_loss, sparse_ho_mincut_loss, unbatched_hosc_orthogonality_loss
    one = i["batch"][i["edge_index"][0]] == 0
    none = i["edge_index"][:, :0]
    return {
        "ortho_mask": hosc_orthogonality_loss(i["s"], i["mask"]),
        "ortho_nomask": hosc_orthogonality_loss(i["s"]),
        "ortho_sum": hosc_orthogonality_loss(i["s"], i["mask"], batch_reduction="sum"),
        "ortho_k1": hosc_orthogonality_loss(i["s"][:, :, :1], i["mask"]),
        "unbatched_ortho": unbatched_hosc_orthogonality_loss(i["s_flat"], i["batch"]),
        "unbatched_ortho_sum": unbatched_hosc_orthogonality_loss(i["s_flat"], i["batch"], batch_reduction="sum"),
        "unbatched_ortho_nobatch": unbatched_hosc_orthogonality_loss(i["s_flat"]),
        "unbatched_ortho_k1": unbatched_hosc_orthogonality_loss(i["s_flat"][:, :1], i["batch"]),
        "ho_w": sparse_ho_mincut_loss(i["edge_index"], i["s_flat"], i["edge_weight"], i["batch"]),
        "ho_u": sparse_ho_mincut_loss(i["edge_index"], i["s_flat"], None, i["batch"]),
        "ho_sum": sparse_ho_mincut_loss(i["edge_index"], i["s_flat"], i["edge_weight"], i["batch"], batch_reduction="sum"),
        "ho_nobatch": sparse_ho_mincut_loss(i["edge_index"][:, one], i["s_flat"][:6], i["edge_weight"][one]),
        "ho_nobatch_sum": sparse_ho_mincut_loss(i["edge_index"][:, one], i["s_flat"][:6], i["edge_weight"][one],
                                                batch_reduction="sum"),
        "ho_no_edges": sparse_ho_mincut_loss(none, i["s_flat"], None, i["batch"]),
        "ho_no_edges_nobatch": sparse_ho_mincut_loss(none, i["s_flat"][:6], None),
    }


def test_float64_loss_forms_match_the_reference():
    c = CASES["hosc_functions_f64"]
    e = c["expected"]
    got = _function_values(c["inputs"])
    assert set(got) == set(e)
    k = c["inputs"]["s"].size(-1)
    for name, v in got.items():
        assert v.dtype == torch.float64 and v.shape == e[name].shape, name
        # the orthogonality loss relative to sqrt(K) / (sqrt(K) - 1), the larger of its two cancelling terms (times the
        # three graphs under "sum"), the motif cut relative to its magnitude
        scale = math.sqrt(k) / (math.sqrt(k) - 1) * (3 if name.endswith("sum") else 1) if "ortho" in name \
            else abs(float(e[name]))
        assert abs(float(v) - float(e[name])) <= 1e-12 * scale, (name, float(v), float(e[name]))


def test_float32_host_tensors_have_no_cpu_fallback():
    from tgp import _native
    from tgp.utils.losses import hosc_orthogonality_loss, sparse_ho_mincut_loss, unbatched_hosc_orthogonality_loss
    s = torch.softmax(torch.randn(2, 5, 3), -1)
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        hosc_orthogonality_loss(s)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        unbatched_hosc_orthogonality_loss(s[0])
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        sparse_ho_mincut_loss(ei, s[0])
