"""SAGPooling's public surface on the CPU: the reference's names, signatures and defaults (poolers/sag.py:104-161),
``repr``, exports, the alias set, PyG's state-dict names, what the one-channel layers refuse, the C ABI of the new
entries, and the host path of the scorer and the selection on every stored fixture.  (Reduce and Connect have no CPU
implementation in this project -- tests/test_abi.py::test_no_cpu_fallback -- so the pooled features are taken from the
restatement's Reduce over the pooler's own selection, and the pooled edges are checked on the device.)"""
import ctypes
import inspect
import os
import re

import pytest
import torch

import sag_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = torch.load(os.path.join(HERE, "golden", "golden_sag_v1.pt"), weights_only=True)["cases"]
NEW_SYMBOLS = ["tgp_row_project2_f32", "tgp_sag_aggregate_f32", "tgp_sag_score_bwd_x_f32"]


def build(c):
    from tgp.poolers import SAGPooling
    p = SAGPooling(GNN=c["gnn"], **c["cfg"]).eval()
    p.load_state_dict(c["params"])
    return p


def test_constructor_and_forward_match_the_reference():
    from tgp.poolers import SAGPooling
    want = [("in_channels", inspect.Parameter.empty), ("ratio", 0.5), ("GNN", None), ("min_score", None),
            ("multiplier", 1.0), ("nonlinearity", "tanh"), ("lift", "precomputed"), ("s_inv_op", "transpose"),
            ("connect_red_op", "sum"), ("lift_red_op", "sum"), ("remove_self_loops", True), ("degree_norm", False),
            ("edge_weight_norm", False), ("kwargs", inspect.Parameter.empty)]
    sig = inspect.signature(SAGPooling.__init__).parameters
    assert [(n, p.default) for n, p in sig.items() if n != "self"] == want
    assert sig["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    fwd = inspect.signature(SAGPooling.forward).parameters
    assert list(fwd) == ["self", "x", "adj", "edge_weight", "so", "batch", "attn", "lifting", "kwargs"]
    assert [fwd[n].default for n in ("adj", "edge_weight", "so", "batch", "attn", "lifting")] == [None] * 5 + [False]
    assert SAGPooling.get_signature().has_kwargs


def test_layers_match_pyg_signatures_and_names():
    from tgp.nn import GraphConv, SAGEConv
    assert [(n, p.default) for n, p in inspect.signature(GraphConv.__init__).parameters.items() if n != "self"] == [
        ("in_channels", inspect.Parameter.empty), ("out_channels", inspect.Parameter.empty), ("aggr", "add"),
        ("bias", True)]
    assert [(n, p.default) for n, p in inspect.signature(SAGEConv.__init__).parameters.items() if n != "self"] == [
        ("in_channels", inspect.Parameter.empty), ("out_channels", inspect.Parameter.empty), ("aggr", "mean"),
        ("root_weight", True), ("bias", True)]
    for cls in (GraphConv, SAGEConv):
        assert list(inspect.signature(cls.forward).parameters) == ["self", "x", "edge_index", "edge_weight"]
    g = GraphConv(5, 1)
    assert {k: tuple(v.shape) for k, v in g.state_dict().items()} == {
        "lin_rel.weight": (1, 5), "lin_rel.bias": (1,), "lin_root.weight": (1, 5)}
    assert sorted(GraphConv(5, 1, bias=False).state_dict()) == ["lin_rel.weight", "lin_root.weight"]
    s = SAGEConv(5, 1)
    assert {k: tuple(v.shape) for k, v in s.state_dict().items()} == {
        "lin_l.weight": (1, 5), "lin_l.bias": (1,), "lin_r.weight": (1, 5)}
    assert sorted(SAGEConv(5, 1, root_weight=False).state_dict()) == ["lin_l.bias", "lin_l.weight"]
    # PyG's Linear default: weights and bias uniform in +-1/sqrt(in_channels)
    torch.manual_seed(0)
    big = GraphConv(400, 1)
    for t in big.state_dict().values():
        assert float(t.abs().max()) <= 0.05
    assert float(big.lin_rel.weight.detach().abs().max()) > 0.04
    before = big.lin_root.weight.clone()
    big.reset_parameters()
    assert not torch.equal(before, big.lin_root.weight)


def test_state_dict_names_and_checkpoints():
    from tgp.poolers import SAGPooling
    for name, c in CASES.items():
        p = build(c)
        assert sorted(p.state_dict()) == sorted(c["params"]), name
    assert sorted(SAGPooling(4).state_dict()) == ["gnn.lin_rel.bias", "gnn.lin_rel.weight", "gnn.lin_root.weight"]
    assert sorted(SAGPooling(4, GNN="sage").state_dict()) == ["gnn.lin_l.bias", "gnn.lin_l.weight", "gnn.lin_r.weight"]
    assert SAGPooling(4).selector.weight is None and SAGPooling(4).selector.in_channels is None


def test_gnn_argument_and_kwargs_filtering():
    import tgp.nn as nn
    from tgp.poolers import SAGPooling
    assert type(SAGPooling(4).gnn) is nn.GraphConv and type(SAGPooling(4, GNN=nn.GraphConv).gnn) is nn.GraphConv
    assert type(SAGPooling(4, GNN="GraphConv").gnn) is nn.GraphConv
    assert type(SAGPooling(4, GNN=nn.SAGEConv).gnn) is nn.SAGEConv and type(SAGPooling(4, GNN="sage").gnn) is nn.SAGEConv
    with pytest.raises(ValueError, match="Unknown GNN"):
        SAGPooling(4, GNN="gcn")
    p = SAGPooling(4, aggr="mean", bias=False, root_weight=False, not_an_argument=3)  # GraphConv has no root_weight
    assert p.gnn.aggr == "mean" and p.gnn.lin_rel.bias is None and hasattr(p.gnn, "lin_root")
    p = SAGPooling(4, GNN="sage", root_weight=False)
    assert not hasattr(p.gnn, "lin_r")
    p = SAGPooling(4, ratio=3, min_score=0.1, multiplier=2.0, nonlinearity="identity", s_inv_op="inverse",
                   connect_red_op="max", lift_red_op="mean", remove_self_loops=False, degree_norm=True,
                   edge_weight_norm=True, lift="transpose")
    assert (p.selector.ratio, p.selector.min_score, p.selector.s_inv_op, p.multiplier) == (3, 0.1, "inverse", 2.0)
    assert p.selector._fused_act == "linear" and SAGPooling(4).selector._fused_act == "tanh"
    c = p.connector
    assert (c.reduce_op, c.remove_self_loops, c.degree_norm, c.edge_weight_norm) == ("max", False, True, True)
    assert (p.lifter.matrix_op, p.lifter.reduce_op) == ("transpose", "mean")
    before = [t.clone() for t in p.gnn.state_dict().values()]
    p.reset_parameters()
    assert not any(torch.equal(a, b) for a, b in zip(before, p.gnn.state_dict().values()))


def test_repr_is_the_reference_one():
    from tgp.poolers import SAGPooling
    r = repr(SAGPooling(4, ratio=0.25, multiplier=2.0, connect_red_op="max"))
    lines = r.split("\n")
    assert lines[0] == "SAGPooling(" and lines[-1] == ")" and lines[-2] == "\tmultiplier=2.0"
    assert lines[1].startswith("\tselect=TopkSelect(in_channels=None, ratio=0.25, act=")
    assert "SparseConnect(reduce_op=max" in lines[4]
    assert SAGPooling(4).extra_repr_args() == {"multiplier": 1.0}


def test_exports_and_alias_set():
    import tgp
    import tgp.nn as nn
    import tgp.poolers as P
    assert "SAGPooling" in P.pooler_classes and "SAGPooling" in P.__all__
    assert P.pooler_classes == sorted(P.pooler_classes)
    # the alias set is pinned to the five poolers of the hot path
    assert sorted(P.pooler_map) == ["diff", "graclus", "mincut", "ndp", "topk"]
    with pytest.raises(ValueError, match="Unknown pooler_name"):
        P.get_pooler("sag", in_channels=4)
    assert nn.__all__ == ["GraphConv", "SAGEConv"] and tgp.nn is nn
    from tgp import functions, kernels
    assert list(inspect.signature(functions.sag_score).parameters) == [
        "x", "edge_index", "w_rel", "w_root", "bias", "mean", "use_tanh"]
    for fn in ("row_project2", "sag_edge_group", "sag_aggregate", "sag_score_bwd_x", "sag_score"):
        assert callable(getattr(kernels, fn)), fn


def test_what_the_layers_do_not_implement_names_the_argument():
    from tgp.nn import GraphConv, SAGEConv
    from tgp.poolers import SAGPooling
    for cls in (GraphConv, SAGEConv):
        with pytest.raises(NotImplementedError, match="out_channels"):
            cls(4, 2)
        with pytest.raises(NotImplementedError, match="aggr"):
            cls(4, 1, aggr="max")
        with pytest.raises(NotImplementedError, match="edge_weight"):
            cls(4, 1)(torch.randn(3, 4), torch.tensor([[0, 1], [1, 2]]), torch.ones(2))
    with pytest.raises(NotImplementedError, match="aggr"):
        SAGPooling(4, aggr="max")


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_scorer_and_selection_reproduce_the_fixture(name):
    """The composed host path of the layer and the selector's host path, as ``SAGPooling.forward`` chains them."""
    from tgp import _native
    c = CASES[name]
    e, i = c["expected"], c["inputs"]
    p = build(c)
    attn = i["x"] if i.get("attn") is None else i["attn"]
    attn = attn.view(-1, 1) if attn.dim() == 1 else attn
    with torch.no_grad():
        raw = p.gnn(attn, i["edge_index"])
        assert raw.shape == (attn.size(0), 1)
        so = p._score_and_select(attn, i["edge_index"], i["batch"])
    torch.testing.assert_close(raw.view(-1), e["score"], rtol=1e-5, atol=1e-5)
    assert torch.equal(so.node_index, e["so"]["node_index"]) and torch.equal(so.cluster_index, e["so"]["cluster_index"])
    assert so.num_nodes == e["so"]["num_nodes"] and so.num_supernodes == e["so"]["num_supernodes"]
    torch.testing.assert_close(so.weight, e["so"]["weight"], rtol=1e-5, atol=1e-5)
    # the restatement's Reduce over the pooler's own selection and weights
    perm = torch.empty_like(so.node_index)
    perm[so.cluster_index] = so.node_index
    w = torch.empty_like(so.weight)
    w[so.cluster_index] = so.weight
    torch.testing.assert_close(p.multiplier * i["x"][perm] * w.view(-1, 1), e["x"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(R.pool_case(c)[4], e["x"], rtol=1e-5, atol=1e-5)
    if i["batch"] is not None:
        assert torch.equal(i["batch"][perm], e["batch"])
    # the whole forward stops where every pooler of this project stops on host tensors: at Reduce
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        p(x=i["x"], adj=i["edge_index"], edge_weight=i["edge_weight"], batch=i["batch"], attn=i.get("attn"))


def test_host_gradients_reach_the_layer():
    c = CASES["sag_graphconv_mean"]
    p = build(c)
    i = c["inputs"]
    x = i["x"].clone().requires_grad_(True)
    so = p._score_and_select(x, i["edge_index"], i["batch"])
    (so.weight ** 2).sum().backward()
    assert x.grad is not None and all(q.grad is not None and float(q.grad.abs().sum()) > 0 for q in p.gnn.parameters())


def test_a_custom_gnn_takes_the_generic_path():
    from tgp.poolers import SAGPooling
    calls = []

    class Mine(torch.nn.Module):
        def __init__(self, in_channels, out_channels, scale=1.0):
            super().__init__()
            self.lin = torch.nn.Linear(in_channels, out_channels)
            self.scale = scale

        def reset_parameters(self):
            self.lin.reset_parameters()

        def forward(self, x, edge_index):
            calls.append((tuple(x.shape), tuple(edge_index.shape)))
            return self.lin(x) * self.scale

    p = SAGPooling(4, GNN=Mine, scale=2.0, aggr="mean").eval()  # (aggr is not Mine's: dropped)
    assert type(p.gnn) is Mine and p.gnn.scale == 2.0 and sorted(p.state_dict()) == ["gnn.lin.bias", "gnn.lin.weight"]
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1, 2], [1, 2, 3]])
    with torch.no_grad():
        so = p._score_and_select(x, ei, None)
        want = torch.tanh(p.gnn.lin(x).view(-1) * 2.0)
    assert calls[0] == ((6, 4), (2, 3))
    assert so.num_supernodes == 3 and torch.equal(so.node_index, torch.sort(torch.topk(want, 3).indices).values)
    torch.testing.assert_close(so.weight, want[so.node_index])


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from tgp import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tgp_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tgp_(?:sag|row_project2)_[a-z0-9_]+)\s*\(", text))
    assert declared == set(NEW_SYMBOLS)
    assert {s for s in _native.SIGNATURES if s.startswith(("tgp_sag_", "tgp_row_project2_"))} == set(NEW_SYMBOLS)
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name
    assert _native.lib().tgp_version() == 10044  # (appended entry points: the ABI number did not move)
    assert "sag_score.hip" in open(os.path.join(ROOT, "torch-geometric-pool_amd", "csrc", "Makefile")).read()


def test_new_entry_points_validate_without_a_gpu():
    from tgp import _native
    lib = _native.lib()
    d = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(d)
    big = 1 << 31
    assert lib.tgp_row_project2_f32(p, 4, 8, 4, p, p, p, p + 16, None) == -1  # row stride below F
    assert b"tgp_row_project2_f32" in lib.tgp_last_error()
    assert lib.tgp_row_project2_f32(None, 4, 8, 8, p, p, p, p + 16, None) == -1
    assert lib.tgp_row_project2_f32(p, 4, 8, 8, p, p, p, p, None) == -1  # one buffer for both outputs
    assert lib.tgp_row_project2_f32(p, 4, 8, 8, p, p, p, None, None) == -1
    assert lib.tgp_row_project2_f32(p, 1, big, big, p, p, p, p + 16, None) == -4
    assert lib.tgp_row_project2_f32(None, 0, 8, 8, None, None, None, None, None) == 0  # no rows: nothing to do
    assert lib.tgp_sag_aggregate_f32(p, None, p, p + 32, None, None, 4, big, 0, 0, None, p, None) == -4  # E > int32
    assert b"tgp_sag_aggregate_f32" in lib.tgp_last_error()
    assert lib.tgp_sag_aggregate_f32(p, None, p, p + 32, None, None, big, 4, 0, 0, None, p, None) == -4
    assert lib.tgp_sag_aggregate_f32(None, None, p, p + 32, None, None, 4, 4, 0, 0, None, p, None) == -1  # no offsets
    assert lib.tgp_sag_aggregate_f32(p, None, None, p + 32, None, None, 4, 4, 0, 0, None, p, None) == -1  # no sources
    assert lib.tgp_sag_aggregate_f32(p, None, p, p + 32, None, None, 4, 4, 0, 0, None, None, None) == -1  # no output
    assert lib.tgp_sag_aggregate_f32(p, None, p, p + 32, None, None, 4, 4, 2, 0, None, p, None) == -1  # mean not 0/1
    assert lib.tgp_sag_aggregate_f32(p, None, p, p + 32, None, None, 4, 4, 0, 3, None, p, None) == -1  # unknown act
    assert lib.tgp_sag_aggregate_f32(p, None, p, p, None, None, 4, 4, 0, 0, None, p, None) == -1  # p as the output
    assert lib.tgp_sag_aggregate_f32(None, None, None, None, None, None, 0, 0, 0, 0, None, None, None) == 0
    assert lib.tgp_sag_score_bwd_x_f32(p, p, p, p, 4, big, 0, p, None) == -4
    assert lib.tgp_sag_score_bwd_x_f32(p, None, p, p, 4, 4, 0, p, None) == -1
    assert b"tgp_sag_score_bwd_x_f32" in lib.tgp_last_error()
    assert lib.tgp_sag_score_bwd_x_f32(p, p, p, p, 4, 4, 1, None, None) == -1
    assert lib.tgp_sag_score_bwd_x_f32(None, None, None, None, 0, 4, 0, None, None) == 0


def test_native_wrappers_refuse_host_tensors():
    from tgp import _native, functions, kernels
    x, ei, w = torch.randn(3, 4), torch.tensor([[0, 1], [1, 2]]), torch.randn(1, 4)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        kernels.row_project2(x, w, w)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        functions.sag_score(x, ei, w, w, None, False, True)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        kernels.sag_score_bwd_x(torch.randn(3), torch.randn(3), w, w)
