"""MaxCutPooling's public surface on the CPU: the reference's names, signatures and defaults (poolers/maxcut.py,
select/maxcut_select.py), ``repr``, exports, the alias set, the reference's state-dict names, the C ABI of the new
entries, and the composed route of the score net, the selection, the assignment and the loss on every stored fixture.
(Reduce and Connect have no CPU implementation in this project -- tests/test_abi.py::test_no_cpu_fallback -- so the
pooled features are taken from the restatement's Reduce over the pooler's own selection, and the pooled edges are checked
on the device.)"""
import ctypes
import inspect
import os
import re

import pytest
import torch

import maxcut_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = torch.load(os.path.join(HERE, "golden", "golden_maxcut_v1.pt"), weights_only=True)["cases"]
POOL = sorted(n for n, c in CASES.items() if c["kind"] == "pool")
NEW_SYMBOLS = ["tgp_maxcut_assign_round_i32", "tgp_maxcut_cut_f32", "tgp_maxcut_degree_f32", "tgp_maxcut_layer_f32",
               "tgp_maxcut_max_width", "tgp_maxcut_tail_f32", "tgp_maxcut_tail_max_params", "tgp_maxcut_wgrad_f32",
               "tgp_maxcut_wgrad_workspace_bytes"]
SELECTOR_UNITS = [32, 32, 32, 32, 16, 16, 16, 16, 8, 8, 8, 8]


def build(c):
    from tgp.poolers import MaxCutPooling
    p = MaxCutPooling(**c["cfg"]).eval()
    p.load_state_dict(c["params"])
    return p


def select(p, c, dtype=torch.float32):
    i = c["inputs"]
    ew = None if i["edge_weight"] is None else i["edge_weight"].to(dtype)
    return p.selector(x=i["x"].to(dtype), edge_index=i["edge_index"], edge_weight=ew, batch=i["batch"])


def test_constructors_and_forward_match_the_reference():
    from tgp.poolers import MaxCutPooling, MaxCutScoreNet, MaxCutSelect
    empty = inspect.Parameter.empty
    net = [("mp_act", "tanh"), ("mlp_units", [16, 16]), ("mlp_act", "relu"), ("act", "tanh"), ("delta", 2.0)]
    want = [("in_channels", empty), ("ratio", 0.5), ("assign_all_nodes", True), ("max_iter", 5), ("loss_coeff", 1.0),
            ("mp_units", [32, 32, 32, 32])] + net + [
        ("lift", "precomputed"), ("s_inv_op", "transpose"), ("connect_red_op", "sum"), ("lift_red_op", "sum"),
        ("remove_self_loops", True), ("degree_norm", False), ("edge_weight_norm", True)]
    sig = inspect.signature(MaxCutPooling.__init__).parameters
    assert [(n, p.default) for n, p in sig.items() if n != "self"] == want
    want = [("in_channels", empty), ("ratio", 0.5), ("assign_all_nodes", True), ("max_iter", 5),
            ("mp_units", SELECTOR_UNITS)] + net + [("min_score", None), ("s_inv_op", "transpose")]
    sig = inspect.signature(MaxCutSelect.__init__).parameters
    assert [(n, p.default) for n, p in sig.items() if n != "self"] == want
    sig = inspect.signature(MaxCutScoreNet.__init__).parameters
    assert [(n, p.default) for n, p in sig.items() if n not in ("self", "kwargs")] == (
        [("in_channels", empty), ("mp_units", SELECTOR_UNITS)] + net)
    assert sig["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    fwd = inspect.signature(MaxCutPooling.forward).parameters
    assert list(fwd) == ["self", "x", "adj", "edge_weight", "so", "batch", "lifting", "kwargs"]
    assert list(inspect.signature(MaxCutSelect.forward).parameters) == ["self", "x", "edge_index", "edge_weight", "batch",
                                                                         "kwargs"]
    p = MaxCutPooling(4, ratio=0.25, loss_coeff=0.5, delta=1.5, max_iter=3)
    assert p.has_loss and p.extra_repr_args() == {"loss_coeff": 0.5}
    assert repr(p).startswith(
        "MaxCutPooling(\n\tselect=MaxCutSelect(in_channels=4, ratio=0.25, assign_all_nodes=True, "
        "mp_units=[32, 32, 32, 32], mp_act='tanh', mlp_units=[16, 16], mlp_act='relu', act='tanh', delta=1.5, "
        "max_iter=3)\n\treduce=BaseReduce()")
    assert repr(p).endswith("\tloss_coeff=0.5\n)")
    assert (p.in_channels, p.ratio, p.assign_all_nodes, p.max_iter, p.delta, p.act) == (4, 0.25, True, 3, 1.5, "tanh")
    c = p.connector
    assert (c.reduce_op, c.remove_self_loops, c.degree_norm, c.edge_weight_norm) == ("sum", True, False, True)
    sel = p.selector
    assert sel.weight is None and sel.in_channels == 4 and sel.score_act == "tanh" and sel.min_score is None
    with pytest.raises(ValueError, match="SelectOutput .so. cannot be None for lifting"):
        p(torch.zeros(2, 4), lifting=True)


def test_state_dict_names_are_the_references_and_the_fixture_round_trips():
    from tgp.nn import GCNConv
    from tgp.poolers import MaxCutPooling
    pre = "selector.score_net."
    assert {k: tuple(v.shape) for k, v in MaxCutPooling(5, mp_units=[8, 6], mlp_units=[3]).state_dict().items()} == {
        pre + "initial_layer.weight": (5, 5), pre + "initial_layer.bias": (5,),
        pre + "mp_convs.0.bias": (8,), pre + "mp_convs.0.lin.weight": (8, 5),
        pre + "mp_convs.1.bias": (6,), pre + "mp_convs.1.lin.weight": (6, 8),
        pre + "mlp.0.weight": (3, 6), pre + "mlp.0.bias": (3,),
        pre + "final_layer.weight": (1, 3), pre + "final_layer.bias": (1,)}
    for name, c in CASES.items():
        p = build(c)
        assert sorted(p.state_dict()) == sorted(c["params"]), name
        for k, v in p.state_dict().items():
            assert torch.equal(v, c["params"][k]), (name, k)
    torch.manual_seed(0)
    conv = GCNConv(300, 200, normalize=False)  # glorot: uniform in +-sqrt(6 / (in + out)); the bias starts at zero
    bound = (6.0 / 500) ** 0.5
    assert 0.9 * bound < float(conv.lin.weight.detach().abs().max()) <= bound and float(conv.bias.detach().abs().max()) == 0.0
    assert sorted(GCNConv(3, 2, normalize=False, bias=False).state_dict()) == ["lin.weight"]
    for kw in (dict(), dict(normalize=True), dict(normalize=False, improved=True),
               dict(normalize=False, add_self_loops=True)):
        with pytest.raises(NotImplementedError, match="GCNConv"):
            GCNConv(3, 2, **kw)
    before = [t.clone() for t in build(CASES["maxcut_default"]).state_dict().values()]
    p = build(CASES["maxcut_default"])
    p.reset_parameters()
    changed = [not torch.equal(a, b) for a, b in zip(before, p.state_dict().values())]
    names = list(p.state_dict())
    # (as in the reference, ``initial_layer`` is not reset; the fixture's biases were drawn, PyG's reset zeroes them)
    assert all(ch for ch, n in zip(changed, names) if "initial_layer" not in n)


def test_exports_and_alias_set():
    import tgp.nn as nn
    import tgp.poolers as P
    import tgp.select as S
    import tgp.utils as U
    from tgp.poolers import maxcut
    assert "MaxCutPooling" in P.pooler_classes and P.pooler_classes == sorted(P.pooler_classes)
    for name in ("MaxCutPooling", "MaxCutSelect", "MaxCutScoreNet"):
        assert name in P.__all__ and name in S.__all__, name
        assert getattr(S, name) is getattr(maxcut, name) and getattr(P, name) is getattr(maxcut, name)
    assert issubclass(S.MaxCutSelect, S.TopkSelect)
    assert sorted(P.pooler_map) == ["diff", "graclus", "mincut", "ndp", "topk"]
    with pytest.raises(ValueError, match="Unknown pooler_name"):
        P.get_pooler("maxcut", in_channels=4)
    assert nn.__all__ == ["GraphConv", "SAGEConv"] and callable(nn.GCNConv)
    assert "delta_gcn_matrix" in U.__all__ and "maxcut_loss" in U.__all__
    from tgp import functions, kernels
    from tgp.utils.losses import maxcut_loss
    assert U.maxcut_loss is maxcut_loss
    for fn in ("maxcut_degree", "maxcut_layer", "maxcut_tail", "maxcut_wgrad", "maxcut_cut", "maxcut_assign_rounds",
               "maxcut_n_p"):
        assert callable(getattr(kernels, fn)), fn
    assert callable(functions.maxcut_score) and callable(functions.maxcut_loss)


@pytest.mark.parametrize("name", POOL)
def test_composed_route_reproduces_the_fixture(name):
    c = CASES[name]
    e, i = c["expected"], c["inputs"]
    p = build(c)
    with torch.no_grad():
        so = select(p, c)
        loss = p.compute_loss(so.scores, i["edge_index"], i["edge_weight"], i["batch"])
    assert sorted(loss) == ["maxcut_loss"]
    torch.testing.assert_close(so.scores, e["scores"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(loss["maxcut_loss"], e["loss"]["maxcut_loss"], rtol=1e-5, atol=1e-5)
    assert torch.equal(so.node_index, e["so"]["node_index"]) and torch.equal(so.cluster_index, e["so"]["cluster_index"])
    assert so.num_supernodes == e["so"]["num_supernodes"] and so.num_nodes == e["so"]["num_nodes"]
    torch.testing.assert_close(so.weight, e["so"]["weight"], rtol=1e-5, atol=1e-5)
    assert "scores" in so._extra_args
    assign_all = c["cfg"].get("assign_all_nodes", True)
    if assign_all:
        assert torch.equal(so.cluster_index, e["cluster_index"]) and so.node_index.numel() == i["x"].size(0)
        kept = e["kept"]
    else:  # the selection itself: the kept nodes in ascending order with their position in the selection
        kept = torch.empty_like(so.node_index)
        kept[so.cluster_index] = so.node_index
        assert torch.equal(kept, e["kept"])
    x_pool = R.reduce(i["x"], so.scores, kept, so.cluster_index if assign_all else None, assign_all)
    torch.testing.assert_close(x_pool, e["x"], rtol=1e-5, atol=1e-5)


def test_composed_route_in_float64_and_its_gradients():
    c = CASES["maxcut_loops_duplicates"]
    f, i = c["f64"], c["inputs"]
    p = build(c).double()
    x = i["x"].double().requires_grad_(True)
    so = p.selector(x=x, edge_index=i["edge_index"], edge_weight=i["edge_weight"].double(), batch=i["batch"])
    loss = p.compute_loss(so.scores, i["edge_index"], i["edge_weight"].double(), i["batch"])["maxcut_loss"]
    torch.testing.assert_close(so.scores, f["scores"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(loss, f["loss"]["maxcut_loss"], rtol=1e-12, atol=1e-12)
    assert torch.equal(so.cluster_index, f["cluster_index"])
    x_pool = R.reduce(x, so.scores, f["kept"], so.cluster_index, True)
    names = f["grads"]["names"]
    par = dict(p.named_parameters())
    grads = torch.autograd.grad((x_pool ** 2).sum() + loss, [x] + [par[k] for k in names], allow_unused=True)
    torch.testing.assert_close(grads[0], f["grads"]["x"], rtol=1e-11, atol=1e-12)
    flat = torch.cat([(torch.zeros_like(par[k]) if g is None else g).reshape(-1) for k, g in zip(names, grads[1:])])
    torch.testing.assert_close(flat, f["grads"]["params_flat"], rtol=1e-11, atol=1e-12)


def test_an_empty_edge_list_and_no_connectivity_at_all():
    c = CASES["maxcut_empty"]
    p = build(c)
    with torch.no_grad():
        so = select(p, c)
        none = p.selector(x=c["inputs"]["x"], edge_index=None, batch=c["inputs"]["batch"])
        loss = p.compute_loss(so.scores, c["inputs"]["edge_index"], None, c["inputs"]["batch"])["maxcut_loss"]
    torch.testing.assert_close(so.scores, c["expected"]["scores"], rtol=1e-5, atol=1e-5)
    assert torch.equal(none.scores, so.scores) and float(loss) == 0.0
    sizes = torch.bincount(c["inputs"]["batch"])
    assert so.num_supernodes == int(torch.ceil(sizes.float() * 0.5).sum())  # top-k only: assign_all_nodes is off


def test_leftover_nodes_land_on_a_kept_node_of_their_own_graph():
    c = CASES["maxcut_leftovers"]
    i = c["inputs"]
    p = build(c)
    torch.manual_seed(0)
    with torch.no_grad():
        so = select(p, c)
    torch.testing.assert_close(so.scores, c["expected"]["scores"], rtol=1e-5, atol=1e-5)
    kept = torch.sort(c["expected"]["kept"])[0]
    assert so.num_supernodes == kept.numel() and so.node_index.numel() == i["x"].size(0)
    want = torch.tensor(R.assign_rounds(kept, i["edge_index"], i["x"].size(0), c["cfg"]["max_iter"]))
    reached = want > 0
    assert 0 < int(reached.sum()) < want.numel()  # the case has leftovers
    assert torch.equal(so.cluster_index[reached], want[reached] - 1)
    assert torch.equal(i["batch"][kept[so.cluster_index]], i["batch"])  # every node inside its own graph


def test_delta_gcn_matrix_and_maxcut_loss_are_the_references_functions():
    from tgp.utils import delta_gcn_matrix, maxcut_loss
    assert list(inspect.signature(delta_gcn_matrix).parameters) == ["edge_index", "edge_weight", "delta", "num_nodes"]
    assert list(inspect.signature(maxcut_loss).parameters) == ["scores", "edge_index", "edge_weight", "batch",
                                                               "batch_reduction"]
    ei = torch.tensor([[0, 1, 1, 2, 0, 1], [1, 0, 2, 1, 1, 1]])  # a duplicate of 0 -> 1 and a self-loop on 1
    w = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 7.0])
    index, value = delta_gcn_matrix(ei, w, delta=2.0, num_nodes=4)
    dense = torch.zeros(4, 4).index_put((index[0], index[1]), value, accumulate=True)
    deg = torch.tensor([6.0, 5.0, 4.0, 0.0])
    a = torch.zeros(4, 4).index_put((ei[0, :5], ei[1, :5]), w[:5], accumulate=True)
    dinv = torch.where(deg > 0, deg.pow(-0.5), torch.zeros(4))
    torch.testing.assert_close(dense, -torch.eye(4) + 2.0 * dinv.view(-1, 1) * a * dinv.view(1, -1))
    assert torch.equal(index, torch.sparse_coo_tensor(index, value, (4, 4)).coalesce().indices())  # coalesced, as given back
    assert delta_gcn_matrix(ei, None)[1].dtype == torch.float32  # the reference's unit weights
    index3, _ = delta_gcn_matrix(ei, w)  # without num_nodes the size comes from the list: no row for node 3
    assert int(index3.max()) == 2
    coo, none = delta_gcn_matrix(torch.sparse_coo_tensor(ei, w, (4, 4)).coalesce(), delta=2.0, num_nodes=4)
    assert none is None and coo.is_sparse
    torch.testing.assert_close(coo.to_dense(), dense)
    s = torch.tensor([0.5, -1.0, 0.25, 2.0])
    batch = torch.tensor([0, 0, 0, 1])
    az = torch.tensor([(1.0 + 5.0) * -1.0, 2.0 * 0.5 + 3.0 * 0.25 + 7.0 * -1.0, 4.0 * -1.0, 0.0])
    want = torch.stack([(s * az)[:3].sum() / w.sum(), torch.tensor(0.0)])  # the graph without edges: volume 0 -> 1
    torch.testing.assert_close(maxcut_loss(s, ei, w, batch), want.mean())
    torch.testing.assert_close(maxcut_loss(s.view(-1, 1), ei, w, batch, "sum"), want.sum())
    torch.testing.assert_close(maxcut_loss(s[:3], ei, None), (s[:3] * torch.tensor([-2.0, -0.25, -1.0])).sum() / 6.0)
    with pytest.raises(ValueError, match="Expected scores to have shape"):
        maxcut_loss(torch.zeros(4, 2), ei, w)


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from tgp import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tgp_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(tgp_maxcut_[a-z0-9_]+)\s*\(", text))) == NEW_SYMBOLS
    assert sorted(s for s in _native.SIGNATURES if s.startswith("tgp_maxcut_")) == NEW_SYMBOLS
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name


def test_new_entry_points_validate_without_a_gpu():
    """Argument validation happens before any HIP call, so it can be exercised without a device."""
    from tgp import _native
    lib = _native.lib()
    buf = (ctypes.c_int64 * 16)()
    p, big = ctypes.addressof(buf), 1 << 31
    assert lib.tgp_maxcut_max_width() == 64 and lib.tgp_maxcut_tail_max_params() == 8192
    assert lib.tgp_maxcut_degree_f32(p, None, p, p, None, 4, 4, None, None, None, None) == -1  # no dinv
    assert b"tgp_maxcut_degree_f32" in lib.tgp_last_error()
    assert lib.tgp_maxcut_degree_f32(p, None, None, p, None, 4, 4, p + 32, None, None, None) == -1  # no sources
    assert lib.tgp_maxcut_degree_f32(p, None, p, p, p + 64, 4, 4, p + 32, p + 64, None, None) == -1  # weights as coef
    assert lib.tgp_maxcut_degree_f32(p, None, p, p, None, 4, 4, p + 32, p + 64, p + 64, None) == -1  # coef twice
    assert lib.tgp_maxcut_degree_f32(p, None, p, p, None, big, 4, p + 32, None, None, None) == -4
    assert lib.tgp_maxcut_degree_f32(p, None, p, p, None, 4, big, p + 32, None, None, None) == -4
    assert lib.tgp_maxcut_degree_f32(None, None, None, None, None, 0, 0, None, None, None, None) == 0  # no nodes
    f = 2.0

    def layer(grp=p, other=p, coef=p, dinv=p, z=p, n=4, e=4, c=8, act=1, h=p + 32, w=None, cn=0, zn=None):
        return lib.tgp_maxcut_layer_f32(grp, None, other, coef, dinv, z, None, n, e, c, None, f, act, h, w, cn, zn, None)

    assert layer(c=65) == -1 and b"tgp_maxcut_layer_f32" in lib.tgp_last_error()  # wider than the kernels take
    assert layer(c=0) == -1 and layer(cn=65, w=p, zn=p + 64) == -1
    assert layer(act=3) == -1  # unknown activation
    assert layer(h=None) == -1  # no output
    assert layer(w=p + 96) == -1 and layer(w=p + 96, cn=4) == -1 and layer(zn=p + 64, cn=4) == -1  # half a projection
    assert layer(h=p) == -1 and layer(w=p + 96, cn=4, zn=p) == -1  # z as an output
    assert layer(dinv=None) == -1 and layer(coef=None) == -1 and layer(grp=None) == -1
    assert layer(n=big) == -4 and layer(e=big) == -4 and layer(n=-1) == -1
    assert layer(grp=None, other=None, coef=None, dinv=None, z=None, n=0, e=0, h=None) == 0  # no nodes
    widths = (ctypes.c_int64 * 2)(16, 16)
    wp = ctypes.addressof(widths)
    need = 8 * 16 + 16 + 16 * 16 + 16 + 16 + 1

    def tail(h=p, n=4, c=8, w=wp, layers=2, params=p, count=need, mlp_act=2, act=1, out=p + 32):
        return lib.tgp_maxcut_tail_f32(h, n, c, w, layers, params, count, mlp_act, act, out, None)

    assert tail(count=need - 1) == -1 and b"tgp_maxcut_tail_f32" in lib.tgp_last_error()  # does not fit the widths
    assert tail(c=65) == -1 and tail(layers=9) == -1 and tail(w=None) == -1
    assert tail(mlp_act=3) == -1 and tail(act=-1) == -1
    assert tail(out=None) == -1 and tail(out=p) == -1 and tail(params=None) == -1
    wide = (ctypes.c_int64 * 2)(64, 65)
    assert tail(w=ctypes.addressof(wide), count=8 * 64 + 64 + 64 * 65 + 65 + 65 + 1) == -1  # a width of 65
    deep = (ctypes.c_int64 * 3)(64, 64, 64)
    assert tail(w=ctypes.addressof(deep), layers=3, c=64, count=3 * (64 * 64 + 64) + 65) == -1  # beyond the LDS budget
    assert tail(n=big) == -4
    assert tail(h=None, n=0, params=None, out=None) == 0  # no rows
    assert lib.tgp_maxcut_wgrad_workspace_bytes(0, 8, 8) >= 8 * 8 * 4
    assert lib.tgp_maxcut_wgrad_workspace_bytes(1025, 64, 64) >= 2 * 64 * 64 * 4
    assert lib.tgp_maxcut_wgrad_workspace_bytes(4, 65, 8) == 0
    assert lib.tgp_maxcut_wgrad_f32(p, p, 4, 8, 8, p + 32, p + 64, 8, None) == -2  # workspace too small
    assert b"workspace too small" in lib.tgp_last_error()
    assert lib.tgp_maxcut_wgrad_f32(p, p, 4, 65, 8, p + 32, p + 64, 1 << 20, None) == -1
    assert lib.tgp_maxcut_wgrad_f32(None, p, 4, 8, 8, p + 32, p + 64, 1 << 20, None) == -1
    assert lib.tgp_maxcut_wgrad_f32(p, p, 4, 8, 8, None, p + 64, 1 << 20, None) == -1
    assert lib.tgp_maxcut_wgrad_f32(p, p, big, 8, 8, p + 32, p + 64, 1 << 20, None) == -4
    assert lib.tgp_maxcut_cut_f32(p, None, p, None, p, 4, 4, None, None, None, None) == -1  # no output
    assert b"tgp_maxcut_cut_f32" in lib.tgp_last_error()
    assert lib.tgp_maxcut_cut_f32(p, None, p, None, p, 4, 4, p, None, None, None) == -1  # s as an output
    assert lib.tgp_maxcut_cut_f32(p, None, None, None, p, 4, 4, p + 32, None, None, None) == -1  # no endpoints
    assert lib.tgp_maxcut_cut_f32(p, None, p, None, None, 4, 4, p + 32, None, None, None) == -1  # no scores
    assert lib.tgp_maxcut_cut_f32(p, None, p, None, p, 4, big, p + 32, None, None, None) == -4
    assert lib.tgp_maxcut_cut_f32(None, None, None, None, None, 0, 0, None, None, None, None) == 0
    assert lib.tgp_maxcut_assign_round_i32(p, None, p, p, 4, 4, p, None) == -1  # one buffer for both label sets
    assert b"tgp_maxcut_assign_round_i32" in lib.tgp_last_error()
    assert lib.tgp_maxcut_assign_round_i32(p, None, p, p, 4, 4, None, None) == -1
    assert lib.tgp_maxcut_assign_round_i32(p, None, None, p, 4, 4, p + 32, None) == -1
    assert lib.tgp_maxcut_assign_round_i32(p, None, p, p, big, 4, p + 32, None) == -4
    assert lib.tgp_maxcut_assign_round_i32(None, None, None, None, 0, 0, None, None) == 0


def test_native_wrappers_refuse_host_tensors():
    from tgp import _native, kernels
    from tgp import functions as Fn
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        kernels.maxcut_wgrad(torch.zeros(4, 3), torch.zeros(4, 2))
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        kernels.maxcut_tail(torch.zeros(4, 3), [torch.zeros(1, 3)], [torch.zeros(1)], "relu", "tanh")
    with pytest.raises(ValueError, match="act 'elu' is not one of"):
        kernels.maxcut_layer(None, ei[0], None, torch.zeros(2), torch.zeros(2, 3), None, None, 2.0, act="elu")
    w = torch.ones(2, requires_grad=True)
    with pytest.raises(RuntimeError, match="gives edge weights no gradient"):
        Fn.maxcut_score(torch.zeros(2, 3), ei, w, (), (), (), (), 2.0, "tanh", "relu", "tanh")
    with pytest.raises(RuntimeError, match="gives edge weights no gradient"):
        Fn.maxcut_loss(torch.zeros(2), ei, w, None, torch.tensor([0, 2]), 1, 2)
    # host tensors never reach a kernel: the score net and the loss take their composed forms
    from tgp.poolers import MaxCutScoreNet
    from tgp.utils.losses import maxcut_loss_native_case
    net = MaxCutScoreNet(3, mp_units=[4], mlp_units=[2])
    assert not net.native_case(torch.zeros(2, 3), ei, None)
    assert not maxcut_loss_native_case(torch.zeros(2), ei, None, None)
    assert MaxCutScoreNet(3, mp_units=[4], mp_act="elu")._native_acts[0] is None  # an activation the kernels do not know
