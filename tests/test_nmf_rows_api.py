"""The row-walking NMF kernel's C ABI on the CPU: the two appended symbols, the argument validation of
``tgp_nmfrows_factorize_f32`` (before any HIP call) and the LDS frame behind ``tgp_nmfrows_lds_nodes``."""
import ctypes
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ["tgp_nmfrows_factorize_f32", "tgp_nmfrows_lds_nodes"]


def test_header_ctypes_table_library_and_wrappers_agree():
    from tgp import _native, kernels
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tgp_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(tgp_nmfrows_[a-z0-9_]+)\s*\(", text))) == NEW_SYMBOLS
    assert sorted(s for s in _native.SIGNATURES if s.startswith("tgp_nmfrows_")) == NEW_SYMBOLS
    handle = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(handle, name) for name in NEW_SYMBOLS)
    assert callable(kernels.nmf_rows_factorize) and callable(kernels.nmf_rows_lds_nodes)
    assert kernels.NMF_NOT_COALESCED == 8


def test_the_lds_frame_fits_and_is_used_up():
    """The documented frame in floats: Gram [32][32], four partial tiles, 16 fold words, 4 control words, then W and H^T
    [n][K | 1]: the limit is the largest n that fits 160 KiB."""
    from tgp import _native
    lib = _native.lib()
    fixed = 32 * 32 + 4 * 32 * 32 + 16 + 4
    for k in (1, 2, 5, 8, 31, 32):
        n = lib.tgp_nmfrows_lds_nodes(k)
        assert 4 * (fixed + 2 * n * (k | 1)) <= 160 * 1024 < 4 * (fixed + 2 * (n + 1) * (k | 1)), k
    assert lib.tgp_nmfrows_lds_nodes(32) > lib.tgp_nmf_max_nodes() == 128
    assert lib.tgp_nmfrows_lds_nodes(0) == 0 and lib.tgp_nmfrows_lds_nodes(lib.tgp_nmf_max_k() + 1) == 0


BUF = (ctypes.c_int64 * 64)()
P = ctypes.addressof(BUF)
GOOD = dict(grp=P, dst=P, gid=P, gptr=P, gperm=P, n=4, e=4, g=2, k=2, cols=2, tol=1e-4, iters=10, w0=None, h0=None,
            s=P + 64, w=P + 128, ht=P + 192, status=P + 256, dgrp=P, src=P, lst=P, listed=1, home=0)


@pytest.mark.parametrize("change, code, word", [
    (dict(k=0), -1, b"K"), (dict(k=33), -1, b"K"), (dict(n=-1), -1, b"negative"), (dict(e=-1), -1, b"negative"),
    (dict(g=-1), -1, b"negative"), (dict(listed=-1), -1, b"negative"), (dict(cols=0), -1, b"out_cols"),
    (dict(iters=0), -1, b"max_iter"), (dict(tol=-1e-3), -1, b"tol"), (dict(tol=float("nan")), -1, b"tol"),
    (dict(home=2), -1, b"home"), (dict(grp=None), -1, b"NULL"), (dict(dgrp=None), -1, b"NULL"),
    (dict(dst=None), -1, b"NULL"), (dict(src=None), -1, b"NULL"), (dict(gid=None), -1, b"NULL"),
    (dict(gptr=None), -1, b"NULL"), (dict(gperm=None), -1, b"NULL"), (dict(s=None), -1, b"NULL"),
    (dict(w=None), -1, b"NULL"), (dict(ht=None), -1, b"NULL"), (dict(status=None), -1, b"NULL"),
    (dict(lst=None), -1, b"NULL"), (dict(w0=P + 320), -1, b"init"), (dict(h0=P + 320), -1, b"init"),
    (dict(n=1 << 31), -4, b"int32"), (dict(e=1 << 31), -4, b"int32"), (dict(g=1 << 31), -4, b"int32"),
    (dict(listed=1 << 31), -4, b"int32"), (dict(listed=0, lst=None), 0, b""),
    (dict(n=0, g=0, e=0, dst=None, src=None), 0, b"")])
def test_the_entry_validates_without_a_gpu(change, code, word):
    from tgp import _native
    lib = _native.lib()
    a = dict(GOOD, **change)
    rc = lib.tgp_nmfrows_factorize_f32(a["grp"], None, a["dst"], None, a["gid"], a["gptr"], a["gperm"], a["n"], a["e"],
                                       a["g"], a["k"], a["cols"], 0, a["tol"], a["iters"], a["w0"], a["h0"], a["s"],
                                       a["w"], a["ht"], None, None, a["status"], a["dgrp"], None, a["src"], a["lst"],
                                       a["listed"], a["home"], None)
    assert rc == code
    if code:
        err = lib.tgp_last_error()
        assert b"tgp_nmfrows_factorize_f32" in err and word in err
