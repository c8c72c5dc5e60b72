"""ctypes binding of libhpvg.so (the C ABI declared in include/hpvg.h).

There is NO CPU fallback: every op of this package runs hand-written gfx950 kernels through this
library.  If the library is missing, or a tensor is not a contiguous fp32 device tensor, the call fails
loudly."""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("HPVG_LIB") or os.path.join(_HERE, "libhpvg.so")  # HPVG_LIB: development builds (tools/trace_conv.py)
HEADER_PATH = os.path.join(_ROOT, "include", "hpvg.h")

_lib = None

_C_TYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t, "unsigned": ctypes.c_uint, "unsigned long long": ctypes.c_ulonglong}


class ScalarPtrs(ctypes.Structure):
    """hpvg_scalar_ptrs: the K <= LOG_MAX_K device scalar pointers of one loss-log row, passed by value."""
    # _fields_ follows below, once the header has given HPVG_LOG_MAX_K


_C_TYPES["hpvg_scalar_ptrs"] = ScalarPtrs


def parse_header(text):
    """({name: (restype, argtypes)}, {HPVG_*: int}) of a header text: every `ret hpvg_name(args);` and every integer
    `#define HPVG_*`.  A parameter that holds `*` is a void pointer, every other type is looked up by name; a declaration
    that is not understood in full is an ImportError, never a guess."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(HPVG_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    sigs = {}
    for stmt in text.split(";"):
        if not re.search(r"\bhpvg_\w+\s*\(", stmt):
            continue
        m = re.fullmatch(r"(?:\s*extern\s*\"C\"\s*\{)?\s*(\w[\w \t]*?)\s+(hpvg_\w+)\s*\(([^()]*)\)\s*", stmt)
        if not m:
            raise ImportError("hpvg.h: declaration not understood: %s" % " ".join(stmt.split()))
        ret, name, params = m.groups()
        if ret not in ("int", "size_t"):
            raise ImportError("hpvg.h: %s returns %r (int or size_t expected)" % (name, ret))
        args = []
        for prm in ([] if params.strip() in ("", "void") else params.split(",")):
            ctype = ctypes.c_void_p if "*" in prm else _C_TYPES.get(" ".join(prm.split()[:-1]))
            if ctype is None:
                raise ImportError("hpvg.h: %s has a parameter of unknown type: %r" % (name, " ".join(prm.split())))
            args.append(ctype)
        sigs[name] = (_C_TYPES[ret], args)
    return sigs, consts


with open(HEADER_PATH) as _f:
    _SIGNATURES, _CONSTANTS = parse_header(_f.read())
LOG_MAX_K = _CONSTANTS["HPVG_LOG_MAX_K"]
PACK_BATCH_MAX = _CONSTANTS["HPVG_PACK_BATCH_MAX"]
SN_BATCH_MAX = _CONSTANTS["HPVG_SN_BATCH_MAX"]
ScalarPtrs._fields_ = [("p", ctypes.c_void_p * LOG_MAX_K)]
_ERR = {v: k for k, v in _CONSTANTS.items() if k.startswith("HPVG_ERR_")}
_RETURNS_SIZE = frozenset(n for n, (ret, _) in _SIGNATURES.items() if ret is ctypes.c_size_t)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "hp-vae-gan_amd: %s not found. Build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
            "This package has no CPU fallback." % LIB_PATH)
    # torch has already loaded its HIP runtime (libamdhip64.so.7); libhpvg.so resolves against that same soname,
    # so stream handles and device pointers are shared with torch.
    lib = ctypes.CDLL(LIB_PATH)
    missing = [name for name in sorted(_SIGNATURES) if not hasattr(lib, name)]
    if missing:
        raise ImportError("libhpvg.so out of sync with include/hpvg.h: missing=%s" % missing)
    for name, (ret, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ret
    _lib = lib
    return lib


def check_symbols():
    """The sorted names declared in include/hpvg.h; load() has found each in the library and bound it."""
    load()
    return sorted(_SIGNATURES)


def stream():
    """hipStream_t of torch's current stream (raw handle lookup: ~0.2 us, vs ~3 us for torch.cuda.current_stream())."""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def ptr(t):
    """Device pointer of a contiguous fp32 device tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("hp-vae-gan_amd: tensor is on %s; these ops run only on an MI355X device (no CPU fallback)" % t.device)
    if t.dtype not in (torch.float32, torch.float64, torch.uint8, torch.int8, torch.int32, torch.int64):  # int32 also carries the 1-bit mask words
        raise RuntimeError("hp-vae-gan_amd: unsupported dtype %s" % t.dtype)
    if not t.is_contiguous():
        raise RuntimeError("hp-vae-gan_amd: tensor must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if name in _RETURNS_SIZE:
        return rc
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (name, _ERR.get(rc, rc)))
    return rc
