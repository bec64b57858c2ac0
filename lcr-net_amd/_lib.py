"""ctypes binding of liblcr_hip.so (C ABI: include/lcr_hip.h), signatures read from the headers.  Loud failure if the library is absent.
Two views: lib().lcr_x(...) returns the code, call.lcr_x(...) raises on a nonzero one; ws() / ws_size() are the workspace query."""
import ctypes
import os
import re
import types

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "liblcr_hip.so")

_lib = None

HEADERS = [os.path.join(_PKG, "..", "include", h) for h in ("lcr_hip.h", "lcr_hip_debug.h")]
_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "unsigned": ctypes.c_uint,
            "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
_RESULTS = {"int": ctypes.c_int, "void": None, "const char*": ctypes.c_char_p}


def parse_header(text):
    """{name: (restype, [argtypes])} of every lcr_* prototype of a header: scalars by _SCALARS, every pointer as c_void_p (tensors,
    struct addresses and byref() objects all pass).  The headers are the only signature table; a prototype this does not
    understand raises and names the function — a guessed or skipped row would corrupt a call frame silently."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    sigs = {}
    for m in re.finditer(r"\b(lcr_\w+)\s*\(", text):
        name = m.group(1)
        head = text[:m.start()]
        res = re.sub(r"\s*\*", "*", " ".join(head[max(head.rfind(c) for c in ";{}") + 1:].split()))
        tail = re.match(r"([^()]*)\)\s*;", text[m.end():])
        if res not in _RESULTS or tail is None:
            raise RuntimeError("%s: cannot parse its prototype (result type %r)" % (name, res))
        args = []
        for p in ([] if tail.group(1).strip() in ("", "void") else tail.group(1).split(",")):
            words = re.sub(r"\bconst\b", " ", p).split()
            ctype = ctypes.c_void_p if "*" in p else _SCALARS.get(" ".join(words[:-1] if len(words) > 1 else words))
            if ctype is None:
                raise RuntimeError("%s: parameter %r has no ctypes mapping" % (name, " ".join(p.split())))
            args.append(ctype)
        sigs[name] = (_RESULTS[res], args)
    return sigs


# entry points that synchronise, compute on the host or issue long launch sequences: called with the interpreter lock RELEASED
_RELEASES_GIL = {"lcr_roformer_forward", "lcr_precompute_batch", "lcr_precompute_batch_rows", "lcr_precompute_batch_rows_ex", "lcr_hashmap_bucket_host", "lcr_encoder_forward", "lcr_encoder_forward_ex", "lcr_ktimer_read",
                 "lcr_ktimer_read2", "lcr_hashmap_order_host", "lcr_ransac_sample_host", "lcr_icp_point_to_point", "lcr_icp_point_to_plane", "lcr_netvlad_forward", "lcr_log_sinkhorn", "lcr_log_sinkhorn_ex",
                 "lcr_local_global_registration", "lcr_local_global_registration_ex", "lcr_retrieval_topk", "lcr_stream_spin"}


def build():
    """Compile the library in-tree (hipcc, gfx950)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_lcr_build", os.path.join(_PKG, "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build()


# int results that are a value, not a code (a record count, a yes / no, the version): never an error, in either view
_RETURNS_VALUE = {"lcr_version", "lcr_kpconv_mask_ok", "lcr_gemm_split_ok", "lcr_ktimer_read", "lcr_ktimer_read2"}


def __getattr__(name):
    """`_lib.call`, the checked view of the library: the functions of lib() under the same names, as second function objects with the
    same argtypes and the same interpreter-lock rule, whose nonzero return code raises RuntimeError with lcr_last_error()'s text
    (ctypes' errcheck hook).  The package calls through this view; lib() is for callers that want the code itself.  It is a plain
    namespace that lib() puts into the module, so this hook runs once, before the library is loaded."""
    if name == "call":
        lib()
        return call
    raise AttributeError(name)


def _raise_on_rc(rc, fn, args):
    if rc:
        check(rc, fn.__name__)
    return rc


def lib():
    """The loaded library, every function declared in include/ bound with its header signature and returning its plain result (the raw
    view; `call` is the checked one).  Raises RuntimeError (never falls back) if it has not been built."""
    global _lib, call
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "liblcr_hip.so not found at %s — build it with `python lcr-net_amd/csrc/build.py` "
                "(there is no CPU fallback for the lcr-net_amd hot path)" % LIB_PATH)
        sigs = {}
        for header in HEADERS:
            with open(header) as f:
                sigs.update(parse_header(f.read()))
        L = ctypes.CDLL(LIB_PATH)
        # Entry points that only enqueue a few launches (5-10 us) are bound through PyDLL, i.e. called WITHOUT releasing the interpreter
        # lock: with two host threads each issuing ~1000 such calls per registration pair, the release / re-acquire around every call
        # turned into a lock hand-off per launch (a futex wake each) and two workers ran SLOWER than one (100 vs 136 pairs/s at one pair
        # per call, profiles/r06_pair_host_profile.log).  Calls that block or issue long launch sequences (_RELEASES_GIL) keep
        # releasing it — those are what the pipelines' threads overlap on.
        K = ctypes.PyDLL(LIB_PATH) if os.environ.get("LCR_CTYPES_KEEP_GIL", "1") != "0" else L
        checked = types.SimpleNamespace()
        for name, (res, args) in sigs.items():
            if not hasattr(L, name):
                continue  # symbol presence is enforced by tests/test_cabi_symbols.py against include/lcr_hip.h
            dll = L if name in _RELEASES_GIL else K
            for view, fn in ((L, getattr(dll, name)), (checked, dll[name])):    # dll[name] is a fresh function object, getattr the cached one
                fn.restype, fn.argtypes = res, args
                if view is checked and res is ctypes.c_int and name not in _RETURNS_VALUE:
                    fn.errcheck = _raise_on_rc
                setattr(view, name, fn)
        _lib, call = L, checked
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().lcr_last_error()
        raise RuntimeError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ""))


def ptr(t):
    """Device pointer of a tensor (or NULL for None)."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream_ptr(device=None):
    """hipStream_t of torch's current stream on `device` as a void pointer.  Straight from the C binding: torch.cuda.current_stream
    builds a Stream object per call (4.5 us, ~200 calls per registration pair)."""
    idx = device.index if isinstance(device, torch.device) else None
    if idx is None:
        idx = torch.cuda.current_device() if not isinstance(device, int) else device
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("lcr-net_amd ops run on the GPU only: got a %s tensor (no CPU fallback)" % t.device)


def workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def ws_size(name, *args):
    """What the size query `name` (a *_ws_bytes / *_ws_floats entry: `args`, then a size_t out-pointer) answers."""
    lib()                                   # `call` exists from the first load on
    n = ctypes.c_size_t(0)
    getattr(call, name)(*args, ctypes.byref(n))
    return n.value


def ws(name, *args, device):
    """The workspace tensor that the size query `name` asks for."""
    return workspace(ws_size(name, *args), device)
