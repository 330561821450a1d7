"""ctypes binding of the tgp HIP library (``include/tgp_hip.h``).

The header is the only statement of the C ABI: the argument and return types of every entry point and the values of
its enums are read from it when this module is imported (:func:`parse_header`), so a new entry point or constant is
declared there and nowhere else.

There is deliberately **no CPU or PyTorch fallback** behind these wrappers: if
``lib/libtgp_hip.so`` is missing, or an operator is handed tensors that do not live on a
ROCm device, the call raises.  PyTorch is used for device memory (outputs and workspaces
come from its caching allocator) and for the current HIP stream, nothing else.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Optional

import torch
from torch import Tensor

_HERE = os.path.dirname(os.path.abspath(__file__))
# TGP_HIP_LIB: load another build of the same library (kernel experiments); never a different implementation
LIB_PATH = os.environ.get("TGP_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libtgp_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "tgp_hip.h")


class TgpNativeError(RuntimeError):
    """Raised when the HIP library is missing or reports a non-zero status, or its header cannot be bound."""


# every kind of parameter and of return value the C ABI uses; a pointer of any type is a c_void_p
_BY_VALUE = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
             "double": ctypes.c_double, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}
_FUNCTION = re.compile(r"([\w\s*]+?)\b(tgp_\w+)\s*\(([^()]*)\)")  # return type, name, parameter list
_ENUM = re.compile(r"enum\s+(\w+)\s*\{([^{}]*)\}")
_ENUMERATOR = re.compile(r"(\w+)\s*=\s*(-?(?:0|[1-9]\d*))")  # an explicit decimal value
_POINTER = re.compile(r"[\w\s*]*\*[\w\s*]*")  # const T* name, T* const* name, ...
_VALUE = re.compile(r"(\w+)(?:\s+\w+)?")  # T or T name


def parse_header(text: str):
    """``(signatures, enums)`` of a C header written the way ``include/tgp_hip.h`` is: between comments and
    preprocessor lines, nothing but ``enum name { A = 1, ... };`` and ``type tgp_name(parameters);``.
    ``signatures``: name -> (restype, [argtypes]); ``enums``: enum name -> {enumerator: value}.  Anything else --
    a by-value type outside ``_BY_VALUE`` / ``_RETURNS``, a function pointer, ``...``, an enumerator without an explicit
    value, text that is no complete declaration -- raises :class:`TgpNativeError`; nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text, n_extern = re.subn(r'extern\s+"C"\s*\{', "", text)
    *statements, rest = text.split(";")
    signatures, enums = {}, {}
    for statement in statements:
        decl = " ".join(statement.split())
        fn, enum = _FUNCTION.fullmatch(decl), _ENUM.fullmatch(decl)
        if fn:
            ret, name, params = fn.groups()
            ret = re.sub(r"\s*\*", "*", ret.strip())
            if ret not in _RETURNS:
                raise TgpNativeError(f"C ABI header: {name} returns '{ret}', which is none of {sorted(_RETURNS)}")
            if name in signatures:
                raise TgpNativeError(f"C ABI header: {name} is declared twice")
            argtypes = []
            for param in [] if params.strip() == "void" else params.split(","):
                value = _VALUE.fullmatch(param.strip())
                if _POINTER.fullmatch(param):
                    argtypes.append(ctypes.c_void_p)
                elif value and value[1] in _BY_VALUE:
                    argtypes.append(_BY_VALUE[value[1]])
                else:
                    raise TgpNativeError(f"C ABI header: {name} has the parameter '{param.strip()}', which is neither a "
                                         f"pointer nor one of {sorted(_BY_VALUE)}")
            signatures[name] = (_RETURNS[ret], argtypes)
        elif enum:
            values = {}
            for item in enum[2].split(","):
                enumerator = _ENUMERATOR.fullmatch(item.strip())
                if not enumerator:
                    raise TgpNativeError(f"C ABI header: enum {enum[1]} has the enumerator '{item.strip()}', which is not "
                                         "'NAME = integer'")
                values[enumerator[1]] = int(enumerator[2])
            enums[enum[1]] = values
        elif decl:
            raise TgpNativeError(f"C ABI header: the declaration '{decl[:120]}' is not understood")
    if rest.split() != ["}"] * n_extern:
        raise TgpNativeError(f"C ABI header: '{' '.join(rest.split())[:120]}' after the last declaration is not understood")
    return signatures, enums


def read_header(path: str):
    """:func:`parse_header` of the file at ``path``."""
    try:
        with open(path) as fh:
            text = fh.read()
    except OSError as err:
        raise TgpNativeError(
            f"C ABI header {path} cannot be read ({err.strerror}): the bindings are derived from it") from err
    return parse_header(text)


# SIGNATURES: name -> (restype, argtypes) of every symbol the header declares; ENUMS: its enums
SIGNATURES, ENUMS = read_header(HEADER_PATH)

_flags = ENUMS["tgp_flags"]
REMOVE_SELF_LOOPS = _flags["TGP_REMOVE_SELF_LOOPS"]
DEGREE_NORM = _flags["TGP_DEGREE_NORM"]
EDGE_WEIGHT_NORM = _flags["TGP_EDGE_WEIGHT_NORM"]
SUM_AXIS_ROWS = _flags["TGP_SUM_AXIS_ROWS"]
EPS_FILTER = _flags["TGP_EPS_FILTER"]
ADJ_TRANSPOSED = _flags["TGP_ADJ_TRANSPOSED"]
NODE_FILTER = _flags["TGP_NODE_FILTER"]
WANT_EDGE_ID = _flags["TGP_WANT_EDGE_ID"]
HUGE_ROWS = _flags["TGP_HUGE_ROWS"]
REDUCE_OPS = {name[len("TGP_"):].lower(): value for name, value in ENUMS["tgp_reduce_op"].items()}
REDUCE_OPS["add"] = REDUCE_OPS["sum"]  # the reference accepts both names

BF16 = ENUMS["tgp_dtype"]["TGP_BF16"]  # the storage types of the *_h16 entries
F16 = ENUMS["tgp_dtype"]["TGP_F16"]
H16_CODES = {torch.bfloat16: BF16, torch.float16: F16}

_lib: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the C-ABI library; raises loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TgpNativeError(
                f"tgp HIP extension not built: {LIB_PATH} is missing. Run `python -c 'import "
                "__graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError here == ABI mismatch: fail loudly
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = lib().tgp_last_error().decode(errors="replace")
        raise TgpNativeError(f"{what} failed with status {status}: {msg}")


def checked(fn, *args) -> None:
    """Call a C-ABI entry point; a non-zero status is reported under the symbol that was called."""
    status = fn(*args)
    if status != 0:
        check(status, fn.__name__)


def require_device(*tensors: Optional[Tensor]) -> torch.device:
    """All given tensors must live on one ROCm device; returns it."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise TgpNativeError(
                "tgp (MI355X build) runs Reduce/Connect only on ROCm device tensors; got a "
                f"{t.device} tensor. Move inputs to 'cuda' - there is no CPU fallback.  (The reference's operators also "
                "accept host tensors, reduce/base_reduce.py:141-155: this build does not.  Remedy: "
                "`pooler.to('cuda')` and `x.to('cuda')`, `edge_index.to('cuda')`, `batch.to('cuda')` before the call; the "
                "results come back on the device.)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise TgpNativeError(f"tensors on different devices: {dev} vs {t.device}")
    if dev is None:
        raise TgpNativeError("no device tensor given")
    return dev


def ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(dev: torch.device) -> int:
    """Handle of torch's CURRENT stream on ``dev`` (what the library launches on).  The raw accessor costs ~0.3 us;
    building a torch.cuda.Stream object per call cost ~6 us, a quarter of the whole launch path of a 21 us kernel."""
    if _raw_stream is not None:
        return _raw_stream(dev.index if dev.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(dev).cuda_stream


def workspace(nbytes: int, dev: torch.device) -> Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def f64c(t: Tensor) -> Tensor:
    """fp64 + contiguous view/copy (the float64 value type of the HBM-bound operators)."""
    if t.dtype != torch.float64:
        t = t.to(torch.float64)
    return t if t.is_contiguous() else t.contiguous()


def f32c(t: Tensor) -> Tensor:
    """fp32 + contiguous view/copy (the dtype the path computes in)."""
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t if t.is_contiguous() else t.contiguous()


def i64c(t: Tensor) -> Tensor:
    if t.dtype != torch.int64:
        t = t.to(torch.int64)
    return t if t.is_contiguous() else t.contiguous()


# optional operands: None stays None (the kernel is handed a null pointer), a tensor goes through f32c / i64c
def opt_f32(t: Optional[Tensor]) -> Optional[Tensor]:
    return None if t is None else f32c(t)


def opt_f32_flat(t: Optional[Tensor]) -> Optional[Tensor]:
    """:func:`opt_f32` of the operand as one vector (edge weights, scores, biases: [n] or [n, 1])."""
    return None if t is None else f32c(t.reshape(-1))


def opt_i64(t: Optional[Tensor]) -> Optional[Tensor]:
    return None if t is None else i64c(t)
