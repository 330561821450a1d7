"""``tgp._native.parse_header`` on small header texts: what it binds, and that it refuses what it does not understand
(a wrong guess would load, run, and show up as a wrong answer or a fault on the device)."""
import ctypes

import pytest

from tgp import _native
from tgp._native import TgpNativeError, parse_header


def signatures(text):
    return parse_header(text)[0]


@pytest.mark.parametrize("c_type, kind", [
    ("const float*", ctypes.c_void_p), ("int64_t", ctypes.c_int64), ("int", ctypes.c_int), ("float", ctypes.c_float),
    ("size_t", ctypes.c_size_t), ("double", ctypes.c_double), ("uint32_t", ctypes.c_uint32), ("uint64_t", ctypes.c_uint64)])
def test_every_parameter_kind(c_type, kind):
    assert signatures(f"int tgp_x({c_type} a);") == {"tgp_x": (ctypes.c_int, [kind])}
    assert signatures(f"int tgp_x(int first, {c_type});") == {"tgp_x": (ctypes.c_int, [ctypes.c_int, kind])}  # unnamed


@pytest.mark.parametrize("c_type, kind", [("int", ctypes.c_int), ("size_t", ctypes.c_size_t), ("int64_t", ctypes.c_int64),
                                          ("const char*", ctypes.c_char_p), ("const char *", ctypes.c_char_p)])
def test_every_return_kind(c_type, kind):
    assert signatures(f"{c_type} tgp_x(void);") == {"tgp_x": (kind, [])}


def test_pointers_of_any_shape_and_a_declaration_over_several_lines():
    text = """
    #ifndef H
    #define H
    #include <stdint.h>
    #ifdef __cplusplus
    extern "C" {
    #endif
    #define TGP_ABI_VERSION 7
    int tgp_first(const int64_t* row,
                  int32_t* const* tables /* NULL ok */,   int64_t
                  n, void* stream);
    size_t tgp_second(
        int64_t n
    );
    #ifdef __cplusplus
    }
    #endif
    #endif
    """
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    assert signatures(text) == {"tgp_first": (ctypes.c_int, [p, p, i64, p]), "tgp_second": (ctypes.c_size_t, [i64])}


def test_comments_produce_no_entry():
    text = """
    /* int tgp_in_block(int a); a stray ) and tgp_x( here
       over two lines */
    // int tgp_in_line(int a); tgp_x( and a stray )
    int tgp_real(int a /* tgp_x( ) */, float b);  // tgp_x( )
    """
    assert signatures(text) == {"tgp_real": (ctypes.c_int, [ctypes.c_int, ctypes.c_float])}


@pytest.mark.parametrize("text, named", [
    ("int tgp_bad(long n);", "long n"),
    ("int tgp_bad(int a, unsigned n);", "unsigned n"),
    ("int tgp_bad(unsigned int n);", "unsigned int n"),
    ("int tgp_bad(struct pair p);", "struct pair p"),
    ("int tgp_bad(const int n);", "const int n"),
    ("int tgp_bad(int a, ...);", "..."),
    ("int tgp_bad(int a[4]);", "int a[4]"),
    ("int tgp_bad();", "''"),
    ("int tgp_bad(void (*callback)(int), int n);", "(*callback)"),
    ("long tgp_bad(int n);", "long"),
    ("unsigned tgp_bad(int n);", "unsigned"),
    ("void tgp_bad(int n);", "void"),
    ("struct pair tgp_bad(int n);", "struct pair"),
    ("float* tgp_bad(int n);", "float*"),
    ("int tgp_bad(int n", "int n"),  # half a declaration: no ')' and no ';'
    ("int tgp_good(int n); int tgp_bad(int n) { return n; }", "return n"),
    ("int tgp_bad(int n); int tgp_bad(int64_t n);", "twice"),
    ("#define TWO \\\n  2\nint tgp_bad(int n);", "2"),  # a macro over two lines
])
def test_what_is_not_understood_is_refused_by_name(text, named):
    with pytest.raises(TgpNativeError) as err:
        parse_header(text)
    assert "tgp_bad" in str(err.value) and named in str(err.value)


def test_enums_need_explicit_integer_values():
    text = """
    enum tgp_status { TGP_OK = 0, TGP_ERR_INVALID = -1, /* bad argument */
                      TGP_ERR_RANGE = -4 };
    enum tgp_bits { TGP_A = 1, TGP_B = 256 };
    int tgp_x(void);
    """
    sigs, enums = parse_header(text)
    assert enums == {"tgp_status": {"TGP_OK": 0, "TGP_ERR_INVALID": -1, "TGP_ERR_RANGE": -4},
                     "tgp_bits": {"TGP_A": 1, "TGP_B": 256}}
    assert list(sigs) == ["tgp_x"]
    for body, named in (("TGP_A = 1, TGP_IMPLICIT", "TGP_IMPLICIT"), ("TGP_A = 1, TGP_B = TGP_A << 1", "TGP_A << 1"),
                        ("TGP_A = 0x10", "0x10"), ("TGP_A = 010", "010")):
        with pytest.raises(TgpNativeError) as err:
            parse_header(f"enum tgp_bad {{ {body} }};")
        assert "tgp_bad" in str(err.value) and named in str(err.value)


def test_a_missing_header_is_named(tmp_path):
    path = str(tmp_path / "include" / "tgp_hip.h")
    with pytest.raises(TgpNativeError) as err:
        _native.read_header(path)
    assert path in str(err.value)


def test_the_module_is_bound_from_the_repository_header():
    assert (_native.SIGNATURES, _native.ENUMS) == _native.read_header(_native.HEADER_PATH)
    assert _native.SIGNATURES["tgp_last_error"] == (ctypes.c_char_p, [])
    assert _native.ENUMS["tgp_status"]["TGP_ERR_RANGE"] == -4
    assert _native.REDUCE_OPS["add"] == _native.REDUCE_OPS["sum"] == _native.ENUMS["tgp_reduce_op"]["TGP_SUM"]
