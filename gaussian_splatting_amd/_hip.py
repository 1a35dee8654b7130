"""Loader for libgsplat_hip.so, the C-ABI library declared in include/gsplat_hip.h.

The product path has no CPU fallback: if the library is missing or a call fails this module
raises.  Build it with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C gaussian_splatting_amd/csrc`.
"""
import ctypes
import functools
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# GSPLAT_HIP_LIB selects another build of the same library (tools only: the instrumented
# libgsplat_hip_stats.so of `make stats`); there is still no fallback if it is missing
LIB_PATH = os.environ.get("GSPLAT_HIP_LIB") or os.path.join(_HERE, "libgsplat_hip.so")

# the one statement of the C ABI (in-tree, as csrc/Makefile assumes): entry points, prototypes and constants come from it
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gsplat_hip.h")


class HipLibraryError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64,
            "size_t": ctypes.c_size_t, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64}


def parse_header(text):
    """-> ({gs_name: (restype, [argtypes])}, {GS_NAME: int}) of a header text.  Every pointer parameter is c_void_p (it
    takes None, an address or a ctypes array), a `const char*` return c_char_p; a scalar type that _SCALARS does not list
    raises HipLibraryError: nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    defines = {m.group(1): int(m.group(2))
               for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(GS_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

    def ctype(decl, where, ret=False):
        words = [w for w in decl.replace("*", " * ").split() if w != "const"]
        if "*" in words and (not ret or words == ["char", "*"]):
            return ctypes.c_char_p if ret else ctypes.c_void_p
        if "*" not in words and words and words[0] in _SCALARS and len(words) <= 2 - ret:   # `type`, or `type name`
            return _SCALARS[words[0]]
        raise HipLibraryError(f"{where} `{' '.join(decl.split())}` has no ctypes mapping")

    protos = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(gs_\w+)\s*\(([^;{)]*)\)\s*;", text):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        params = [] if params in ("", "void") else params.split(",")
        protos[name] = (ctype(ret, f"{name}: return type", ret=True),
                        [ctype(p, f"{name}: parameter {i + 1}") for i, p in enumerate(params)])
    return protos, defines


@functools.lru_cache(maxsize=None)
def _header():
    if not os.path.exists(HEADER_PATH):
        raise HipLibraryError(f"{HEADER_PATH} not found: the prototypes of the C ABI are read from it (no untyped calls)")
    with open(HEADER_PATH) as fh:
        return parse_header(fh.read())


def __getattr__(name):
    """EXPORTS (every entry point the header declares) and the header's integer constants (GS_F32, GS_SORT_PREFIX,
    GS_BACKWARD_EXACT, ...), read on first use rather than at import"""
    protos, defines = _header()
    if name != "EXPORTS" and name not in defines:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    return globals().setdefault(name, sorted(protos) if name == "EXPORTS" else defines[name])


def ptr(t):
    """a tensor's device address for a pointer parameter of the C ABI; None -> NULL"""
    return None if t is None else t.data_ptr()


def set_backward_mode(mode):
    """"compat" (default: the reference's arithmetic including SURVEY.md Q1) or "exact" (global splat index
    in the transmittance update: the mathematically exact gradient).  Sets the process-wide DEFAULT: the
    render-backward entry points take the mode per call (ABI 5) and the fused frames pass the default that
    was in force at their FORWARD, so changing it never affects a backward that is already queued"""
    defines = _header()[1]
    code = {"compat": defines["GS_BACKWARD_COMPAT"], "exact": defines["GS_BACKWARD_EXACT"]}.get(mode, mode)
    check(lib().gs_set_backward_mode(int(code)))


def get_backward_mode():
    return int(lib().gs_get_backward_mode())


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                f"{LIB_PATH} not found: the HIP extension is not built. "
                "Run `make -C gaussian_splatting_amd/csrc` (there is no CPU fallback).")
        # One HIP runtime per process: the library needs libamdhip64.so.7 and must bind to the copy
        # PyTorch ships (same SONAME), whose streams and allocations it works on.  Loaded before torch
        # it would pull in /opt/rocm's runtime instead, and the second runtime to initialise finds no
        # device ("no ROCm-capable device is detected").
        import torch  # noqa: F401
        protos = _header()[0]
        loaded = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in protos.items():   # no call without its prototype
            fn = getattr(loaded, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = loaded
    return _lib


def current_stream():
    """torch's current stream on the current device as a ctypes pointer for the C ABI.  The raw-handle query
    (~1 us); torch.cuda.current_stream() builds a Stream object and costs ~15 us of host time per call."""
    import torch

    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def check(status):
    if status != 0:
        raise RuntimeError(lib().gs_last_error().decode())


# ---- optional per-entry-point timing (bench.py) --------------------------------------------------------
# When enabled, every C-ABI call is bracketed by events recorded on torch's current stream -- the
# stream the kernels are launched on -- so the elapsed time of one entry point is the GPU time of
# the kernels it enqueues.
_timers = None
_event_pool = []   # timing events are recycled: creating one costs ~5 us of host time per call
# modules that time their own C-ABI calls the same way (the native frame orchestration,
# csrc/frame_hip.cpp): enable_timing / reserve_events / collect_timing are forwarded to them
timing_providers = []


def _event():
    import torch

    return _event_pool.pop() if _event_pool else torch.cuda.Event(enable_timing=True)


def reserve_events(n):
    """create the timing events ahead of the timed region"""
    import torch

    while len(_event_pool) < n:
        _event_pool.append(torch.cuda.Event(enable_timing=True))
    for p in timing_providers:
        p.reserve_events(n)


_only = None   # name of the one entry point to time, or None for all


def enable_timing(on=True, only=None):
    """only: time just this entry point (two events per frame instead of two per C-ABI call)"""
    global _timers, _only
    _timers = {} if on else None
    _only = only if on else None
    for p in timing_providers:
        p.enable_timing(bool(on), only or "")


def collect_timing():
    """-> {entry point: [ms, ...]} for the calls made since enable_timing(); synchronises."""
    import torch

    torch.cuda.synchronize()
    out = {}
    for name, pairs in (_timers or {}).items():
        out[name] = [a.elapsed_time(b) for a, b in pairs]
        for a, b in pairs:
            _event_pool.append(a)
            _event_pool.append(b)
    if _timers is not None:
        _timers.clear()
    for p in timing_providers:
        for name, ms in p.collect_timing().items():
            out.setdefault(name, []).extend(ms)
    return out


def timed_region(name, fn):
    """run fn() and, when timing is enabled, book its GPU time (events on the current stream) under
    `name` next to the C-ABI entry points -- used for the RCCL collectives of the multi-GPU frame"""
    if _timers is None or (_only is not None and _only != name):
        return fn()
    a, b = _event(), _event()
    a.record()
    out = fn()
    b.record()
    _timers.setdefault(name, []).append((a, b))
    return out


def call(name, *args, label=None):
    """label: the name the call's GPU time is booked under (default: the entry point's) -- a step that one general
    entry serves in every mode keeps one name in the timings"""
    fn = getattr(lib(), name)
    label = label or name
    if _timers is None or (_only is not None and _only != label):
        check(fn(*args))
        return
    a, b = _event(), _event()
    a.record()
    check(fn(*args))
    b.record()
    _timers.setdefault(label, []).append((a, b))
