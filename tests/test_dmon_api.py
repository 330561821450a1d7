"""DMoN's public surface on the CPU: the reference's names, signatures and defaults (poolers/dmon.py:98-116,
utils/losses.py:435-473, 1083-1265), the module's state-dict names, and the float64 loss forms against the reference's
float64 values (tests/golden/golden_dmon_v1.pt) at 1e-12."""
import inspect
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_dmon_v1.pt"), weights_only=True)["cases"]


def test_constructor_matches_the_reference():
    from tgp.poolers import DMoNPooling
    sig = inspect.signature(DMoNPooling.__init__)
    want = [("in_channels", inspect.Parameter.empty), ("k", inspect.Parameter.empty), ("act", None), ("dropout", 0.0),
            ("spectral_loss_coeff", 1.0), ("cluster_loss_coeff", 1.0), ("ortho_loss_coeff", 0.0),
            ("remove_self_loops", True), ("degree_norm", True), ("edge_weight_norm", False), ("adj_transpose", True),
            ("lift", "precomputed"), ("s_inv_op", "transpose"), ("batched", True), ("sparse_output", False),
            ("cache_preprocessing", False)]
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self"]
    assert got == want


def test_exports_and_alias_set():
    import tgp.poolers as P
    assert "DMoNPooling" in P.pooler_classes and "DMoNPooling" in P.__all__
    assert "dmon" not in P.pooler_map  # the alias is a follow-up (the alias set is pinned to five poolers)
    from tgp.utils import losses
    for name, params in (
        ("spectral_loss", ["adj", "S", "adj_pooled", "mask", "num_supernodes", "batch_reduction"]),
        ("cluster_loss", ["S", "mask", "num_supernodes", "batch_reduction"]),
        ("sparse_spectral_loss", ["edge_index", "S", "edge_weight", "batch", "batch_reduction"]),
        ("unbatched_cluster_loss", ["S", "batch", "batch_reduction"]),
    ):
        assert list(inspect.signature(getattr(losses, name)).parameters) == params, name


def test_state_dict_names_and_repr_args():
    from tgp.poolers import DMoNPooling
    for name in ("dmon_batched_default_w", "dmon_batched_mlp2_w", "dmon_u_single_graph"):
        c = CASES[name]
        p = DMoNPooling(**c["cfg"], batched=c["alias"] == "dmon")
        assert sorted(p.state_dict()) == sorted(c["params"]), name
        p.load_state_dict(c["params"])
    p = DMoNPooling(in_channels=5, k=4, ortho_loss_coeff=0.5, batched=False)
    assert p.extra_repr_args() == {"batched": False, "spectral_loss_coeff": 1.0, "cluster_loss_coeff": 1.0,
                                   "ortho_loss_coeff": 0.5}


def test_float64_loss_forms_match_the_reference():
    from tgp.utils.losses import cluster_loss, sparse_spectral_loss, spectral_loss, unbatched_cluster_loss
    c = CASES["dmon_functions_f64"]
    i, e = c["inputs"], c["expected"]
    one = i["batch"][i["edge_index"][0]] == 0
    got = {
        "spectral_mask": spectral_loss(i["adj"], i["s"], i["raw"], i["mask"]),
        "spectral_nomask": spectral_loss(i["adj"], i["s"], i["raw"]),
        "cluster_mask": cluster_loss(i["s"], mask=i["mask"]),
        "cluster_nomask": cluster_loss(i["s"]),
        "cluster_sum": cluster_loss(i["s"], mask=i["mask"], batch_reduction="sum"),
        "sparse_spectral_w": sparse_spectral_loss(i["edge_index"], i["s_flat"], i["edge_weight"], i["batch"]),
        "sparse_spectral_u": sparse_spectral_loss(i["edge_index"], i["s_flat"], None, i["batch"]),
        "sparse_spectral_nobatch": sparse_spectral_loss(i["edge_index"][:, one], i["s_flat"][:6], i["edge_weight"][one]),
        "unbatched_cluster": unbatched_cluster_loss(i["s_flat"], i["batch"]),
        "unbatched_cluster_nobatch": unbatched_cluster_loss(i["s_flat"]),
    }
    for k, v in got.items():
        assert v.dtype == torch.float64, k
        # the spectral loss relative to its larger cancelling term (at most 1 here: S is a softmax, so
        # trace(S^T A S) <= sum(A) = 2m), the cluster loss relative to its magnitude
        scale = 1.0 if "spectral" in k else abs(float(e[k]))
        assert abs(float(v) - float(e[k])) <= 1e-12 * scale, (k, float(v), float(e[k]))


def test_float32_host_tensors_have_no_cpu_fallback():
    from tgp import _native
    from tgp.utils.losses import cluster_loss, unbatched_cluster_loss
    s = torch.softmax(torch.randn(2, 5, 3), -1)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        cluster_loss(s)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        unbatched_cluster_loss(s[0])
