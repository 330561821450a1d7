"""The C ABI of the 16-bit storage kernels (csrc/sparse_half.hip), checked without a GPU: the four entries and the two
dtype codes are bound from the header, and every entry refuses a bad call with its status before any HIP call."""
import ctypes

import pytest

from tgp import _native

V, I64, I, SZ = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
SIGNATURES = {
    "tgp_reduce_sparse_h16": [I, V, I64, I64, I64, V, V, V, V, I64, I64, V, V],
    "tgp_reduce_one_to_one_h16": [I, V, I64, I64, I64, V, I, I64, V, V],
    "tgp_segment_aggr_h16": [I, V, I64, I64, I64, V, I64, V, V, V, V, V, I64, I64, I64, I, V, V, V, V, SZ, V],
    "tgp_segment_aggr_bwd_h16": [I, V, V, I64, I64, I64, V, I64, V, V, V, V, I64, I, V, V],
}
INVALID, WORKSPACE = -1, -2


def test_entries_and_dtype_codes_are_bound_from_the_header():
    assert (_native.BF16, _native.F16) == (1, 2) and _native.ENUMS["tgp_dtype"] == {"TGP_BF16": 1, "TGP_F16": 2}
    lib = _native.lib()
    for name, argtypes in SIGNATURES.items():
        assert _native.SIGNATURES[name] == (ctypes.c_int, argtypes), name
        assert getattr(lib, name).argtypes == argtypes


@pytest.mark.parametrize("code", [_native.BF16, _native.F16])
def test_bad_calls_are_refused_with_their_status(code):
    lib = _native.lib()
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    SUM = 1 << _native.REDUCE_OPS["sum"]

    def reduce(dtype=code, x=p, n=4, out=p):
        return lib.tgp_reduce_sparse_h16(dtype, x, n, 8, 8, p, None, p, p, 4, 2, out, None)

    def one_to_one(dtype=code, pack=p, k=2):
        return lib.tgp_reduce_one_to_one_h16(dtype, p, 4, 8, 8, pack, 1, k, p, None)

    def readout(dtype=code, out=p, rows=600, ws=None, ws_bytes=0):
        return lib.tgp_segment_aggr_h16(dtype, p, rows, 8, 8, p, 0, None, None, None, None, None, 0, 1, 600, SUM, out,
                                        None, None, ws, ws_bytes, None)

    def backward(dtype=code, dx=p, rows=4):
        return lib.tgp_segment_aggr_bwd_h16(dtype, p, p, rows, 8, 8, p, 0, None, p, None, None, 1, SUM, dx, None)

    for call in (reduce, one_to_one, readout, backward):
        assert call(dtype=0) == INVALID and call(dtype=3) == INVALID  # a bad dtype code
        assert b"_h16" in lib.tgp_last_error()
    assert reduce(out=None) == INVALID and reduce(x=None) == INVALID and reduce(n=-1) == INVALID
    assert one_to_one(pack=None) == INVALID and one_to_one(k=-1) == INVALID
    assert readout(out=None) == INVALID and readout(rows=-1) == INVALID
    assert backward(dx=None) == INVALID and backward(rows=-1) == INVALID
    # one segment of 600 rows takes the split route: its fp32 partial records need the workspace of the fp32 entry
    need = lib.tgp_segment_aggr_workspace_bytes(1, 8, SUM, 600)
    assert need > 0
    assert readout(ws=None) == WORKSPACE and readout(ws=p, ws_bytes=need - 1) == WORKSPACE
    assert b"workspace too small" in lib.tgp_last_error()
