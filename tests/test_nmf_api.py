"""NMFPooling's public surface on the CPU: the reference's names, signatures, defaults, ``repr``s and warning
(poolers/nmf.py, select/nmf_select.py), the exports, the alias set, the C ABI of the new entries, and the refusal of host
tensors."""
import ctypes
import inspect
import os
import re
import warnings

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ["tgp_nmf_factorize_f32", "tgp_nmf_init_f32", "tgp_nmf_max_k", "tgp_nmf_max_nodes"]


def params(fn):
    return [(n, p.default) for n, p in inspect.signature(fn).parameters.items() if n not in ("self", "kwargs")]


def test_constructors_and_forward_match_the_reference():
    from tgp.poolers import NMFPooling
    from tgp.select import NMFSelect, nmf_select
    empty = inspect.Parameter.empty
    extras = [("seed", 0), ("tol", 1e-4), ("max_iter", 5000)]
    assert params(NMFPooling.__init__) == [
        ("k", empty), ("cached", False), ("remove_self_loops", True), ("degree_norm", True), ("edge_weight_norm", False),
        ("adj_transpose", True), ("lift", "precomputed"), ("s_inv_op", "transpose"), ("batched", False),
        ("sparse_output", False), ("cache_preprocessing", False)] + extras
    assert params(NMFSelect.__init__) == [("k", empty), ("s_inv_op", "transpose")] + extras
    kinds = inspect.signature(NMFPooling.__init__).parameters
    assert all(kinds[n].kind is inspect.Parameter.KEYWORD_ONLY for n, _ in extras)
    assert all(inspect.signature(NMFSelect.__init__).parameters[n].kind is inspect.Parameter.KEYWORD_ONLY
               for n, _ in extras)
    assert list(inspect.signature(NMFPooling.forward).parameters) == [
        "self", "x", "adj", "edge_weight", "so", "mask", "batch", "batch_pooled", "lifting", "kwargs"]
    assert list(inspect.signature(NMFPooling.precoarsening).parameters) == [
        "self", "edge_index", "edge_weight", "batch", "num_nodes", "kwargs"]
    sel = inspect.signature(NMFSelect.forward).parameters
    assert list(sel) == ["self", "edge_index", "edge_weight", "batch", "num_nodes", "fixed_k", "kwargs"]
    assert sel["batch"].kind is inspect.Parameter.KEYWORD_ONLY and sel["fixed_k"].default is False
    fn = inspect.signature(nmf_select).parameters
    assert list(fn)[:5] == ["edge_index", "k", "edge_weight", "batch", "num_nodes"]
    assert [(n, fn[n].default) for n in ("fixed_k", "seed", "tol", "max_iter", "init", "return_factors")] == [
        ("fixed_k", False), ("seed", 0), ("tol", 1e-4), ("max_iter", 5000), ("init", None), ("return_factors", False)]
    assert all(fn[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("fixed_k", "seed", "init", "return_factors"))
    assert NMFSelect.is_dense is True


def test_reprs_classes_and_the_batched_warning():
    from tgp.connect import DenseConnect
    from tgp.lift import BaseLift
    from tgp.poolers import NMFPooling
    from tgp.reduce import BaseReduce
    from tgp.select import NMFSelect
    from tgp.src import BasePrecoarseningMixin, DenseSRCPooling
    p = NMFPooling(k=4, cached=True, sparse_output=True, seed=3)
    assert repr(p.selector) == "NMFSelect(k=4, s_inv_op=transpose)" and p.selector.seed == 3
    assert repr(p) == ("NMFPooling(\n\tselect=NMFSelect(k=4, s_inv_op=transpose)\n\treduce=BaseReduce()\n"
                       "\tlift=BaseLift(matrix_op=precomputed, reduce_op=sum)\n"
                       "\tconnect=DenseConnect(remove_self_loops=True, degree_norm=True, adj_transpose=True, "
                       "edge_weight_norm=False, sparse_output=True)\n\tbatched=False\n\tcached=True\n)")
    assert isinstance(p, BasePrecoarseningMixin) and isinstance(p, DenseSRCPooling)
    assert isinstance(p.selector, NMFSelect) and type(p.reducer) is BaseReduce and type(p.lifter) is BaseLift
    assert type(p.connector) is DenseConnect and type(p.preconnector) is DenseConnect
    assert p.preconnector.sparse_output is True and p.extra_repr_args() == {"batched": False, "cached": True}
    with pytest.warns(UserWarning, match="NMFPooling does not support dense padded batched inputs"):
        q = NMFPooling(k=2, batched=True)
    assert q.batched is False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        NMFPooling(k=2)


def test_exports_and_the_alias_set():
    import tgp.poolers as P
    import tgp.select as S
    from tgp import kernels
    from tgp.poolers import nmf
    assert "NMFPooling" in P.pooler_classes and P.pooler_classes == sorted(P.pooler_classes)
    for mod, names in ((P, ["NMFPooling", "NMFSelect"]), (S, ["NMFSelect", "nmf_select"])):
        for name in names:
            assert name in mod.__all__ and getattr(mod, name) is getattr(nmf, name), (mod.__name__, name)
    assert sorted(P.pooler_map) == ["diff", "graclus", "mincut", "ndp", "topk"]
    with pytest.raises(ValueError, match="Unknown pooler_name"):
        P.get_pooler("nmf", k=3)
    for fn in ("nmf_factorize", "nmf_init", "nmf_max_nodes", "nmf_max_k"):
        assert callable(getattr(kernels, fn)), fn
    assert (kernels.NMF_BAD_INPUT, kernels.NMF_NON_FINITE, kernels.NMF_OVER_LIMIT) == (1, 2, 4)


def test_host_tensors_and_bad_arguments_are_refused():
    from tgp import _native
    from tgp.poolers import NMFPooling
    from tgp.select import NMFSelect, nmf_select
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    x = torch.randn(3, 2)
    p = NMFPooling(k=2)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        p(x=x, adj=ei)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        NMFSelect(k=2)(ei, batch=torch.zeros(3, dtype=torch.long))
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        nmf_select(ei, 2, torch.ones(4))
    with pytest.raises(ValueError, match="k must be at least 1"):
        nmf_select(ei, 0)
    with pytest.raises(ValueError, match="max_iter"):
        nmf_select(ei, 2, max_iter=0)
    with pytest.raises(ValueError, match="tol"):
        nmf_select(ei, 2, tol=-1.0)
    with pytest.raises(ValueError, match="cannot be None for precoarsening"):
        p.precoarsening()


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from tgp import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tgp_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(tgp_nmf_[a-z0-9_]+)\s*\(", text))) == NEW_SYMBOLS
    assert sorted(s for s in _native.SIGNATURES if s.startswith("tgp_nmf_")) == NEW_SYMBOLS
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name
    m = re.search(r"#define\s+TGP_ABI_VERSION\s+(\d+)", open(os.path.join(ROOT, "include", "tgp_hip.h")).read())
    assert _native.lib().tgp_version() == int(m.group(1))  # (appended entry points: the number the older tests pin stays)


def test_new_entry_points_validate_without_a_gpu():
    """Null pointers, negative sizes, K < 1, max_iter < 1 and tol < 0 are refused before any HIP call, so this runs without
    a device."""
    from tgp import _native
    lib = _native.lib()
    buf = (ctypes.c_int64 * 64)()
    p, big = ctypes.addressof(buf), 1 << 31
    max_n, max_k = lib.tgp_nmf_max_nodes(), lib.tgp_nmf_max_k()
    assert (max_n, max_k) == (128, 32)

    def fact(grp=p, dst=p, gid=p, gptr=p, gperm=p, n=4, e=4, g=2, k=2, cols=2, mn=4, tol=1e-4, iters=10, w0=None, h0=None,
             s=p + 64, status=p + 256):
        return lib.tgp_nmf_factorize_f32(grp, None, dst, None, gid, gptr, gperm, n, e, g, k, cols, mn, 0, tol, iters, w0, h0,
                                         s, None, None, None, None, status, None)

    assert fact(k=0) == -1 and b"tgp_nmf_factorize_f32" in lib.tgp_last_error() and b"K" in lib.tgp_last_error()
    assert fact(n=-1) == -1 and fact(e=-1) == -1 and fact(g=-1) == -1 and fact(cols=0) == -1
    assert fact(iters=0) == -1 and b"max_iter" in lib.tgp_last_error()
    assert fact(tol=-1e-3) == -1 and b"tol" in lib.tgp_last_error() and fact(tol=float("nan")) == -1
    assert fact(grp=None) == -1 and fact(dst=None) == -1 and fact(gid=None) == -1 and fact(gptr=None) == -1
    assert fact(gperm=None) == -1 and fact(s=None) == -1 and fact(status=None) == -1
    assert fact(w0=p + 128) == -1 and fact(h0=p + 128) == -1  # one half of an explicit init
    assert fact(mn=0) == -1 and fact(mn=max_n + 1) == -1
    assert fact(n=big) == -4 and fact(e=big) == -4 and fact(g=big) == -4
    assert fact(n=0, g=0, e=0, dst=None) == 0  # nothing to do

    def init(grp=p, dst=p, gid=p, gptr=p, gperm=p, n=4, e=4, g=2, k=2, mn=4, w0=p + 64, h0=p + 128, status=p + 256):
        return lib.tgp_nmf_init_f32(grp, None, dst, None, gid, gptr, gperm, n, e, g, k, mn, 0, w0, h0, status, None)

    assert init(k=0) == -1 and b"tgp_nmf_init_f32" in lib.tgp_last_error()
    assert init(n=-1) == -1 and init(e=-1) == -1 and init(g=-1) == -1 and init(mn=0) == -1 and init(mn=max_n + 1) == -1
    assert init(grp=None) == -1 and init(dst=None) == -1 and init(gid=None) == -1 and init(gptr=None) == -1
    assert init(gperm=None) == -1 and init(w0=None) == -1 and init(h0=None) == -1 and init(status=None) == -1
    assert init(n=big) == -4 and init(n=0, g=0, e=0, dst=None) == 0
