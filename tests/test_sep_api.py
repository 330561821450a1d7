"""SEP pooling's public surface and its host route: the reference's names, signatures and defaults (poolers/sep.py,
select/sep_select.py), the host-route selector against every stored case of the reference
(tests/golden/golden_sep_v1.pt) on CPU tensors, the refusals, caching and the exports.

Reduce, Connect and Lift have no CPU fallback in this build, so the checks of the pooled outputs through the host-route
selection are marked ``gpu``: the selection is taken on the host, the rest of the pooler runs on the device."""
import ctypes
import inspect
import os

import pytest
import torch

import sep_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_sep_v1.pt"), weights_only=True)["cases"]
TOL = dict(rtol=1e-5, atol=1e-5)


def host_select(c):
    from tgp.select import SEPSelect
    i = c["inputs"]
    return SEPSelect()(edge_index=i["edge_index"], edge_weight=i["edge_weight"], batch=i["batch"],
                       num_nodes=i["x"].size(0))


# ------------------------------------------------------------------------------------------------ CPU
def test_constructors_match_the_reference():
    from tgp.poolers import SEPPooling
    from tgp.select import SEPSelect
    want = [("lift", "precomputed"), ("s_inv_op", "transpose"), ("connect_red_op", "sum"), ("lift_red_op", "sum"),
            ("cached", False), ("remove_self_loops", True), ("degree_norm", True), ("edge_weight_norm", False)]
    got = [(n, p.default) for n, p in inspect.signature(SEPPooling.__init__).parameters.items() if n != "self"]
    assert got == want
    got = [(n, p.default) for n, p in inspect.signature(SEPSelect.__init__).parameters.items() if n != "self"]
    assert got == [("s_inv_op", "transpose")]
    fwd = inspect.signature(SEPPooling.forward).parameters
    assert list(fwd)[:7] == ["self", "x", "adj", "edge_weight", "so", "batch", "lifting"] and fwd["lifting"].default is False


def test_exports_alias_set_and_repr():
    import tgp.poolers as P
    import tgp.select as S
    assert "SEPPooling" in P.pooler_classes and "SEPPooling" in P.__all__
    assert P.pooler_classes == sorted(P.pooler_classes)
    assert sorted(P.pooler_map) == ["diff", "graclus", "mincut", "ndp", "topk"]  # the "sep" alias is a follow-up
    with pytest.raises(ValueError, match="Unknown pooler_name"):
        P.get_pooler("sep")
    for name in ("SEPSelect", "sep_select"):
        assert name in S.__all__ and hasattr(S, name), name
    assert S.SEPSelect is P.SEPSelect
    p = P.SEPPooling()
    assert repr(p.selector) == "SEPSelect()"
    assert p.extra_repr_args() == {"cached": False} and "cached=False" in repr(p) and "SparseConnect" in repr(p)
    assert p.connector.degree_norm is True and p.connector.remove_self_loops is True
    assert not list(p.parameters())


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_route_gives_the_reference_labels(name):
    c = CASES[name]
    so = host_select(c)
    assert so.__dict__["_sep_route"] == "host"
    assert so.num_supernodes == c["expected"]["num_supernodes"] and so.num_nodes == c["inputs"]["x"].size(0)
    assert torch.equal(so.cluster_index, c["expected"]["cluster_index"])
    assert torch.equal(so.node_index, torch.arange(so.num_nodes))


def test_host_route_takes_float64_weights_and_an_unsorted_batch():
    from tgp.select import sep_select
    c = CASES["sep_weighted"]
    i = c["inputs"]
    so = sep_select(i["edge_index"], i["edge_weight"].double(), i["batch"])
    assert torch.equal(so.cluster_index, c["expected"]["cluster_index"])
    n = i["x"].size(0)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))  # node v becomes perm[v]: an unsorted batch vector
    batch = torch.empty_like(i["batch"])
    batch[perm] = i["batch"]
    so = sep_select(perm[i["edge_index"]], i["edge_weight"], batch)
    want, k = R.sep_select(n, perm[i["edge_index"]].numpy(), i["edge_weight"].numpy(), batch.numpy())
    assert so.num_supernodes == k == c["expected"]["num_supernodes"] and so.cluster_index.tolist() == want.tolist()


def test_levels_beyond_one_are_refused_not_rolled_out():
    from tgp.poolers import SEPPooling
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    p = SEPPooling()
    for levels in (2, 3):
        with pytest.raises(NotImplementedError, match="levels > 1"):
            p.multi_level_precoarsening(levels, edge_index=ei, num_nodes=3)
        with pytest.raises(NotImplementedError, match="levels > 1"):
            p.selector.multi_level_select(edge_index=ei, num_nodes=3, levels=levels)
    with pytest.raises(ValueError, match="'levels' must be >= 1"):
        p.multi_level_precoarsening(0, edge_index=ei, num_nodes=3)
    with pytest.raises(ValueError, match="'levels' must be >= 1"):
        p.selector.multi_level_select(edge_index=ei, num_nodes=3, levels=0)
    with pytest.raises(ValueError, match="edge_index cannot be None"):
        p.multi_level_precoarsening(1)
    assert len(p.selector.multi_level_select(edge_index=ei, num_nodes=3, levels=1)) == 1


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_bad_weights_raise(bad):
    from tgp.select import sep_select
    ei = torch.tensor([[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2]])
    w = torch.tensor([1.0, 1.0, bad, 0.5, 1.0, 1.0])
    with pytest.raises(ValueError, match="finite and non-negative"):
        sep_select(ei, w, None, 4)
    # what counts is the sum over duplicates: -1 + 2 on the same pair is a weight of 1 (and 0.5 from the other direction)
    ei2 = torch.tensor([[0, 1, 1, 1, 2], [1, 0, 2, 2, 1]])
    assert sep_select(ei2, torch.tensor([1.0, 1.0, -1.0, 2.0, 0.5]), None, 3).num_supernodes >= 1


def test_other_refusals_and_edge_cases():
    from tgp.select import sep_select
    with pytest.raises(ValueError, match="two graphs"):
        sep_select(torch.tensor([[0, 2], [2, 0]]), None, torch.tensor([0, 0, 1, 1]))
    with pytest.raises(ValueError, match="out of range"):
        sep_select(torch.tensor([[0, 5], [5, 0]]), None, None, 3)
    with pytest.raises(ValueError, match="Expected batch"):
        sep_select(torch.tensor([[0, 1], [1, 0]]), None, torch.tensor([0, 0]), 3)
    with pytest.raises(ValueError, match="route"):
        sep_select(torch.tensor([[0, 1], [1, 0]]), None, None, 2, route="fast")
    with pytest.raises(ValueError, match="route='native'"):
        sep_select(torch.tensor([[0, 1], [1, 0]]), None, None, 2, route="native")
    so = sep_select(torch.zeros(2, 0, dtype=torch.long), None, None, 0)
    assert so.num_nodes == 0 and so.num_supernodes == 0
    so = sep_select(torch.zeros(2, 0, dtype=torch.long), None, torch.tensor([0, 0, 2, 2, 2]))  # edgeless, graph 1 empty
    assert so.cluster_index.tolist() == [0, 1, 2, 3, 4]
    so = sep_select(torch.tensor([[0, 1, 3, 3], [1, 0, 3, 4]]), None, torch.tensor([0, 0, 2, 2, 2]))
    assert so.cluster_index.tolist() == [0, 1, 2, 3, 4] and so.num_supernodes == 5  # two-node components: two singletons
    so = sep_select(torch.tensor([[0, 1], [1, 2]]), torch.tensor([0.0, 1.0]), None, 3)  # a zero entry is "not adjacent"
    assert so.cluster_index.tolist() == [0, 1, 2]


def test_cached_reuses_the_selection():
    from tgp.poolers import SEPPooling
    c = CASES["sep_single_graph"]
    i = c["inputs"]
    p = SEPPooling(cached=True)
    so1 = p.select(edge_index=i["edge_index"], edge_weight=i["edge_weight"], batch=None, num_nodes=30)
    so2 = p.select(edge_index=i["edge_index"][:, :4], edge_weight=None, batch=None, num_nodes=30)
    assert so2 is so1
    p.clear_cache()
    assert p.select(edge_index=i["edge_index"], edge_weight=i["edge_weight"], batch=None, num_nodes=30) is not so1
    q = SEPPooling()
    assert q.select(edge_index=i["edge_index"], num_nodes=30) is not q.select(edge_index=i["edge_index"], num_nodes=30)


def test_entry_points_validate_without_a_gpu():
    from tgp import _native, kernels
    lib = _native.lib()
    limit = lib.tgp_sep_max_nodes()
    assert 128 <= limit <= 256 and kernels.sep_max_nodes() == limit
    d = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(d)
    args = lambda max_n, n=4: (p, None, p, None, p, p, None, p, p, n, 4, 1, max_n, p, p, p, p, None)  # noqa: E731
    assert lib.tgp_sep_select_f32(*args(limit + 1)) == -1 and b"tgp_sep_select_f32" in lib.tgp_last_error()
    assert lib.tgp_sep_select_f32(*args(0)) == -1
    assert lib.tgp_sep_select_f32(*args(8, 1 << 31)) == -4
    assert lib.tgp_sep_select_f32(None, None, p, None, p, p, None, p, p, 4, 4, 1, 8, p, p, p, p, None) == -1


# ------------------------------------------------------------------------------------------------ device operators
def on_device(c):
    d = torch.device("cuda:0")
    i = c["inputs"]
    return (i["x"].to(d), i["edge_index"].to(d), None if i["edge_weight"] is None else i["edge_weight"].to(d),
            None if i["batch"] is None else i["batch"].to(d))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_route_pooler_gives_the_reference_outputs(name):
    from tgp.poolers import SEPPooling
    from tgp.select import SelectOutput
    c = CASES[name]
    want = c["expected"]
    x, ei, ew, batch = on_device(c)
    host = host_select(c)
    so = SelectOutput(cluster_index=host.cluster_index.to(x.device), num_nodes=host.num_nodes,
                      num_supernodes=host.num_supernodes)
    pool = SEPPooling(**c["cfg"])
    out = pool(x=x, adj=ei, edge_weight=ew, so=so, batch=batch)
    assert out.so is so
    torch.testing.assert_close(out.x.cpu(), want["x"], **TOL)
    assert torch.equal(out.edge_index.cpu(), want["edge_index"])
    if want["edge_weight"] is None:  # (unweighted input, no normalisation: the reference returns no weights)
        assert out.edge_weight is None
    else:
        torch.testing.assert_close(out.edge_weight.cpu(), want["edge_weight"], **TOL)
    assert torch.equal(out.batch.cpu(), want["batch"]) if want["batch"] is not None else out.batch is None
    lifted = pool(x=out.x, so=out.so, lifting=True)
    torch.testing.assert_close(lifted.cpu(), want["x_lifted"], **TOL)


@pytest.mark.gpu
def test_precoarsening_equals_the_forward_selection_on_the_host_route():
    from tgp.poolers import SEPPooling
    c = CASES["sep_weighted"]
    x, ei, ew, batch = on_device(c)
    pool = SEPPooling()
    pre = pool.precoarsening(edge_index=ei, edge_weight=ew, batch=batch, num_nodes=x.size(0), route="host")
    (multi,) = pool.multi_level_precoarsening(1, edge_index=ei, edge_weight=ew, batch=batch, num_nodes=x.size(0),
                                              route="host")
    for got in (pre, multi):
        assert got.so.__dict__["_sep_route"] == "host"
        assert torch.equal(got.so.cluster_index.cpu(), c["expected"]["cluster_index"])
        assert torch.equal(got.edge_index.cpu(), c["expected"]["edge_index"])
        torch.testing.assert_close(got.edge_weight.cpu(), c["expected"]["edge_weight"], **TOL)
        assert torch.equal(got.batch.cpu(), c["expected"]["batch"])
