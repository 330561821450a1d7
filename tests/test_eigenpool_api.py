"""EigenPooling's public surface on the CPU: the reference's names, signatures, defaults, ``repr``s and warnings
(poolers/eigenpool.py, select/eigenpool_select.py, reduce/eigenpool_reduce.py, connect/eigenpool_conn.py,
lift/eigenpool_lift.py), the exports, the alias set, the C ABI of the new entries, and the refusal of host tensors."""
import ctypes
import inspect
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ["tgp_eigenpool_lift_f32", "tgp_eigenpool_max_group_nodes", "tgp_eigenpool_modes_f32",
               "tgp_eigenpool_reduce_f32"]


def params(fn):
    return [(n, p.default) for n, p in inspect.signature(fn).parameters.items() if n not in ("self", "kwargs")]


def test_constructors_and_forward_match_the_reference():
    from tgp.connect import EigenPoolConnect
    from tgp.lift import EigenPoolLift
    from tgp.poolers import EigenPooling
    from tgp.reduce import EigenPoolReduce
    from tgp.select import EigenPoolSelect
    empty = inspect.Parameter.empty
    assert params(EigenPooling.__init__) == [
        ("k", empty), ("num_modes", 5), ("normalized", True), ("cached", False), ("remove_self_loops", True),
        ("degree_norm", True), ("edge_weight_norm", False), ("adj_transpose", True), ("lift", "precomputed"),
        ("s_inv_op", "transpose"), ("batched", False), ("sparse_output", False), ("cache_preprocessing", False)]
    assert params(EigenPoolSelect.__init__) == [("k", empty), ("s_inv_op", "transpose"), ("num_modes", 5),
                                                ("normalized", True)]
    assert params(EigenPoolReduce.__init__) == [("num_modes", 5), ("reduce_op", "sum")]
    assert params(EigenPoolLift.__init__) == [("num_modes", 5), ("reduce_op", "sum")]
    assert params(EigenPoolConnect.__init__) == [("remove_self_loops", True), ("degree_norm", True),
                                                 ("adj_transpose", True), ("edge_weight_norm", False),
                                                 ("sparse_output", False)]
    assert list(inspect.signature(EigenPooling.forward).parameters) == [
        "self", "x", "adj", "edge_weight", "so", "mask", "batch", "batch_pooled", "lifting", "kwargs"]
    assert list(inspect.signature(EigenPooling.precoarsening).parameters) == [
        "self", "edge_index", "edge_weight", "batch", "num_nodes", "kwargs"]
    sel = inspect.signature(EigenPoolSelect.forward).parameters
    assert list(sel) == ["self", "x", "edge_index", "edge_weight", "batch", "num_nodes", "kwargs"]
    assert sel["batch"].kind is inspect.Parameter.KEYWORD_ONLY and sel["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    red = inspect.signature(EigenPoolReduce.forward).parameters
    assert list(red) == ["self", "x", "so", "batch", "edge_index", "edge_weight", "return_batched", "kwargs"]
    assert red["batch"].kind is inspect.Parameter.KEYWORD_ONLY and red["return_batched"].default is False
    assert list(inspect.signature(EigenPoolLift.forward).parameters) == [
        "self", "x_pool", "so", "batch", "batch_pooled", "edge_index", "edge_weight", "kwargs"]
    con = inspect.signature(EigenPoolConnect.forward).parameters
    assert list(con) == ["self", "edge_index", "so", "edge_weight", "batch", "batch_pooled", "kwargs"]
    assert con["edge_weight"].kind is inspect.Parameter.KEYWORD_ONLY


def test_reprs_attributes_and_the_two_warnings():
    from tgp.connect import DenseConnect, EigenPoolConnect
    from tgp.poolers import EigenPooling
    from tgp.src import BasePrecoarseningMixin, DenseSRCPooling
    p = EigenPooling(k=4, num_modes=3, normalized=False, cached=True, sparse_output=True)
    assert repr(p) == ("EigenPooling(\n\tselect=EigenPoolSelect(k=4)\n\treduce=EigenPoolReduce(num_modes=3)\n"
                       "\tlift=EigenPoolLift(num_modes=3)\n\tconnect=EigenPoolConnect(remove_self_loops=True, "
                       "degree_norm=True, adj_transpose=True, edge_weight_norm=False, sparse_output=True)\n"
                       "\tbatched=False\n\tk=4\n\tnum_modes=3\n\tnormalized=False\n\tcached=True\n)")
    assert isinstance(p, BasePrecoarseningMixin) and isinstance(p, DenseSRCPooling) and issubclass(EigenPoolConnect, DenseConnect)
    assert p.is_dense and not p.has_loss and not p.is_trainable and p.is_precoarsenable
    assert (p.k, p.num_modes, p.normalized, p.cached, p.batched, p.sparse_output) == (4, 3, False, True, False, True)
    assert p.selector.is_dense and (p.selector.k, p.selector.num_modes, p.selector.normalized) == (4, 3, False)
    assert p.preconnector.sparse_output and p.preconnector.adj_transpose and not p.connector.edge_weight_norm
    with pytest.warns(UserWarning, match="does not support dense padded batched inputs"):
        q = EigenPooling(k=2, batched=True)
    assert q.batched is False
    with pytest.warns(UserWarning, match="ignores the 'lift' argument"):
        EigenPooling(k=2, lift="inverse")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        EigenPooling(k=2)


def test_exports_sorted_classes_and_the_unchanged_alias_set():
    import tgp.connect as C
    import tgp.lift as L
    import tgp.poolers as P
    import tgp.reduce as Rd
    import tgp.select as S
    from tgp.poolers import eigenpool
    assert "EigenPooling" in P.pooler_classes and P.pooler_classes == sorted(P.pooler_classes)
    for mod, names in ((P, ["EigenPooling", "EigenPoolSelect", "EigenPoolReduce", "EigenPoolConnect", "EigenPoolLift"]),
                       (S, ["EigenPoolSelect", "eigenpool_select", "eigenpool_theta"]), (Rd, ["EigenPoolReduce"]),
                       (C, ["EigenPoolConnect"]), (L, ["EigenPoolLift"])):
        for name in names:
            assert name in mod.__all__ and getattr(mod, name) is getattr(eigenpool, name), (mod.__name__, name)
    assert sorted(P.pooler_map) == ["diff", "graclus", "mincut", "ndp", "topk"]
    with pytest.raises(ValueError, match="Unknown pooler_name"):
        P.get_pooler("eigen", k=3)
    from tgp import functions, kernels
    for fn in ("eigenpool_modes", "eigenpool_reduce", "eigenpool_lift", "eigenpool_max_group_nodes"):
        assert callable(getattr(kernels, fn)), fn
    assert callable(functions.eigenpool_reduce) and callable(functions.eigenpool_lift)


def test_empty_graph_and_host_tensors():
    from tgp import _native, kernels
    from tgp.poolers import EigenPooling
    from tgp.select import EigenPoolSelect, SelectOutput
    with pytest.raises(ValueError, match="Cannot perform eigenpool selection on empty graph"):
        EigenPoolSelect(k=2)(edge_index=torch.zeros(2, 0, dtype=torch.long))
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    x = torch.randn(3, 2)
    p = EigenPooling(k=2)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        p(x=x, adj=ei)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        p.selector(edge_index=ei, labels=torch.tensor([0, 0, 1]))
    so = SelectOutput(s=torch.eye(3)[:, :2], theta=torch.zeros(3, 10))
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        p.reducer(x, so)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        p.lifter(torch.zeros(2, 10), so)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        p.connector(ei, so)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        kernels.eigenpool_reduce(torch.zeros(3, 2), kernels.AssignIndex(None, None, 3, 3, device="cpu"), x)
    with pytest.raises(ValueError, match="cannot be None for precoarsening"):
        p.precoarsening()


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from tgp import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tgp_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(tgp_eigenpool_[a-z0-9_]+)\s*\(", text))) == NEW_SYMBOLS
    assert sorted(s for s in _native.SIGNATURES if s.startswith("tgp_eigenpool_")) == NEW_SYMBOLS
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name
    m = re.search(r"#define\s+TGP_ABI_VERSION\s+(\d+)", open(os.path.join(ROOT, "include", "tgp_hip.h")).read())
    assert _native.lib().tgp_version() == int(m.group(1))  # (appended entry points: the number the older tests pin stays)


def test_new_entry_points_validate_without_a_gpu():
    """Null pointers, negative sizes and H < 1 are refused before any HIP call, so this runs without a device."""
    from tgp import _native
    lib = _native.lib()
    buf = (ctypes.c_int64 * 32)()
    p, big = ctypes.addressof(buf), 1 << 31
    limit = lib.tgp_eigenpool_max_group_nodes()
    assert limit == 96

    def modes(grp=p, dst=p, gid=p, tptr=p, tperm=p, n=4, e=4, g=2, h=3, max_m=4, theta=p + 64, status=p + 128):
        return lib.tgp_eigenpool_modes_f32(grp, None, dst, None, gid, tptr, tperm, n, e, g, h, max_m, 1, 0, theta, None,
                                           status, None)

    assert modes(h=0) == -1 and b"tgp_eigenpool_modes_f32" in lib.tgp_last_error() and b"H" in lib.tgp_last_error()
    assert modes(h=-2) == -1 and modes(n=-1) == -1 and modes(e=-1) == -1 and modes(g=-1) == -1
    assert modes(grp=None) == -1 and modes(dst=None) == -1 and modes(gid=None) == -1 and modes(tptr=None) == -1
    assert modes(tperm=None) == -1 and modes(theta=None) == -1 and modes(status=None) == -1
    assert modes(max_m=0) == -1 and modes(max_m=limit + 1) == -1
    assert modes(n=big) == -4 and modes(e=big) == -4 and modes(g=big) == -4
    assert modes(n=0, g=0, e=0, dst=None) == 0  # nothing to do

    def reduce(theta=p, tptr=p, tperm=p, x=p + 64, ldx=4, n=4, g=2, h=3, f=4, max_len=0, out=p + 128):
        return lib.tgp_eigenpool_reduce_f32(theta, tptr, tperm, x, ldx, n, g, h, f, max_len, out, None)

    assert reduce(h=0) == -1 and b"tgp_eigenpool_reduce_f32" in lib.tgp_last_error()
    assert reduce(n=-1) == -1 and reduce(g=-1) == -1 and reduce(f=-1) == -1 and reduce(max_len=-1) == -1
    assert reduce(theta=None) == -1 and reduce(tptr=None) == -1 and reduce(tperm=None) == -1 and reduce(x=None) == -1
    assert reduce(out=None) == -1 and reduce(ldx=3) == -1 and reduce(out=p + 64) == -1  # x as the output
    assert reduce(n=big) == -4 and reduce(g=big) == -4 and reduce(f=big, ldx=big) == -4
    assert reduce(g=0) == 0 and reduce(f=0, ldx=0) == 0

    def lift(theta=p, gid=p, xp=p + 64, n=4, g=2, h=3, f=4, out=p + 128):
        return lib.tgp_eigenpool_lift_f32(theta, gid, xp, n, g, h, f, out, None)

    assert lift(h=0) == -1 and b"tgp_eigenpool_lift_f32" in lib.tgp_last_error()
    assert lift(n=-1) == -1 and lift(g=-1) == -1 and lift(f=-1) == -1
    assert lift(theta=None) == -1 and lift(gid=None) == -1 and lift(xp=None) == -1 and lift(out=None) == -1
    assert lift(out=p + 64) == -1  # x_pool as the output
    assert lift(n=big) == -4 and lift(g=big) == -4 and lift(f=big) == -4
    assert lift(n=0) == 0 and lift(f=0) == 0
