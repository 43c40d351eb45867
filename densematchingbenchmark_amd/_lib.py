"""ctypes binding of libdmb_hip.so -- the only way the Python host layer reaches the HIP kernels.

PyTorch is plumbing here: it owns device memory (``tensor.data_ptr()``) and the current HIP stream
(``torch.cuda.current_stream().cuda_stream``); everything that computes lives behind the C ABI of
``include/dmb_hip.h``.  That header is the only statement of the ABI: the ctypes table (``SIGNATURES``), the ABI version and the
``DMB_*`` constants are read from it at import, and ``launch`` marshals every call from the parsed prototype.  There is NO
fallback: if the library is missing or a tensor is not a CUDA/HIP tensor, the call raises.
"""
import ctypes
import os
import re

import torch  # imported first on purpose: the library then binds to the HIP runtime torch already loaded

_PKG = os.path.dirname(os.path.abspath(__file__))
# DMB_LIB=dev (development scripts only): the build with the kernel-variant switches, lib/libdmb_hip_dev.so (build.py dev=True)
DEV_BUILD = os.environ.get("DMB_LIB", "").startswith("dev")    # "dev" or "dev_<tag>" (a build-time experiment, build.py)
LIB_PATH = os.path.join(_PKG, "lib", "libdmb_hip_%s.so" % os.environ["DMB_LIB"] if DEV_BUILD else "libdmb_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "dmb_hip.h")


class DmbLibraryError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------- the header is the table
_HI = ctypes.POINTER(ctypes.c_int)  # host int array
_HF = ctypes.POINTER(ctypes.c_float)  # host float array
_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = ("void", "float", "double", "int", "long long", "unsigned char")   # what a device pointer may point at


def _ctype(ctype, name, decl):
    """The ctypes type of one C type of the header; ``name``: the parameter's (None: a return type)."""
    words = [w for w in ctype.replace("*", " * ").split() if w != "const"]
    base, stars = " ".join(w for w in words if w != "*"), words.count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base == "char":
        return ctypes.c_char_p
    if name is not None and name.endswith("_host"):     # a HOST array (dmb_hip.h, boundary rules)
        if stars == 1 and base in ("int", "float"):
            return _HI if base == "int" else _HF
    elif stars and name is not None and base in _POINTEES:
        return ctypes.c_void_p      # a device pointer, a host array of device pointers, the stream
    raise DmbLibraryError("include/dmb_hip.h: no ctypes type for `%s` in `%s`" % (" ".join((ctype + " " + (name or "")).split()), decl))


def parse_header(text):
    """``(prototypes, defines)`` of the text of include/dmb_hip.h: entry point -> (restype, [(ctype, parameter name), ...]) and
    DMB_* -> int for every integer ``#define``.  A ``dmb_*`` declaration it cannot map raises -- none is skipped."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    defines = {m.group(1): int(m.group(2), 0)
               for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(DMB_\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', " ", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    protos = {}
    for decl in (" ".join(d.split()) for d in text.split(";")):
        if not re.search(r"\bdmb_\w+\s*\(", decl):
            continue
        m = re.fullmatch(r"([\w \*]+?)\s*\b(dmb_\w+)\s*\(([^()]*)\)", decl)
        if m is None:
            raise DmbLibraryError("include/dmb_hip.h: cannot parse the declaration `%s`" % decl)
        params = []
        for p in ([] if m.group(3).strip() in ("", "void") else m.group(3).split(",")):
            pm = re.fullmatch(r"\s*(.*?[\s\*])(\w+)\s*", p)
            if pm is None:
                raise DmbLibraryError("include/dmb_hip.h: cannot parse the parameter `%s` of `%s`" % (p.strip(), decl))
            params.append((_ctype(pm.group(1), pm.group(2), decl), pm.group(2)))
        protos[m.group(2)] = (_ctype(m.group(1), None, decl), params)
    return protos, defines


PROTOTYPES, DEFINES = parse_header(open(HEADER_PATH).read())
SIGNATURES = {name: (res, [t for t, _ in params]) for name, (res, params) in PROTOTYPES.items()}   # name -> (restype, argtypes)
ABI_VERSION = DEFINES["DMB_ABI_VERSION"]
DECONV3D_WORKSPACE_BYTES = DEFINES["DMB_DECONV3D_WORKSPACE_BYTES"]
CONV_SINGLE_CHAIN = DEFINES["DMB_CONV_SINGLE_CHAIN"]
CONV3D_HEAD_PACKED_FLOATS = DEFINES["DMB_CONV3D_HEAD_PACKED_FLOATS"]
DEEPPRUNER_LOSS_WORKSPACE_DOUBLES = DEFINES["DMB_DEEPPRUNER_LOSS_WORKSPACE_DOUBLES"]


def header_symbols():
    """Every entry point declared in include/dmb_hip.h (used by the CPU-side export test)."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dmb_[a-z0-9_]+)\s*\(", text)))


_lib = None


def load():
    """Load libdmb_hip.so (once).  Raises DmbLibraryError -- never falls back to another implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DmbLibraryError(
            "libdmb_hip.so is not built (%s). Run `python -m densematchingbenchmark_amd.build` "
            "(or __graft_entry__.build()); there is no CPU/PyTorch fallback for this path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.dmb_abi_version() != ABI_VERSION:
        raise DmbLibraryError("%s reports ABI version %d, this binding is written for %d: rebuild it (python -m "
                              "densematchingbenchmark_amd.build)" % (LIB_PATH, lib.dmb_abi_version(), ABI_VERSION))
    tagged = DEV_BUILD and os.environ["DMB_LIB"] != "dev"     # (a build-time experiment: its defines are not known here)
    if not tagged:
        from . import build
        want, got = build.sources_digest(dev=DEV_BUILD), (lib.dmb_build_id() or b"").decode()
        if want != got:
            raise DmbLibraryError("%s was built from other sources than the ones next to it (build id %s..., sources %s...): "
                                  "rebuild it (python -m densematchingbenchmark_amd.build)" % (LIB_PATH, got[:12], want[:12]))
    if DEV_BUILD:
        lib.dmb_dev_set_option.restype = None
        lib.dmb_dev_set_option.argtypes = [ctypes.c_int, ctypes.c_int]
    _lib = lib
    return lib


_shim = None
_shim_state = "untried"      # "untried" | "loaded" | the reason it is not in use


def shim():
    """The thin torch extension over the same C ABI (csrc/torch_shim.cpp -> lib/_dmb_torch_shim.so: unwraps tensors, takes the
    current HIP stream from c10, raises DmbLibraryError on a non-zero code) for the entry points on the per-pair launch path, or
    None -- then ``launch`` below calls them through ctypes, as it calls every other entry point: the SAME functions of the SAME
    library, only more interpreter time per launch (profiles/r06_binding_overhead.log).  Refused (-> None) unless it was built from
    the csrc/torch_shim.cpp / dmb_hip.h / torch next to it and linked against the library that is loaded.  DMB_SHIM=0: never;
    DMB_SHIM=require: raise instead of returning None."""
    global _shim, _shim_state
    if _shim_state != "untried":
        return _shim
    mode = os.environ.get("DMB_SHIM", "auto")
    try:
        if mode == "0":
            raise DmbLibraryError("disabled by DMB_SHIM=0")
        if DEV_BUILD:
            raise DmbLibraryError("the development library is bound through ctypes only")
        lib = load()
        path = os.path.join(_PKG, "lib", "_dmb_torch_shim.so")
        if not os.path.exists(path):
            raise DmbLibraryError("%s is not built (python -m densematchingbenchmark_amd.build --shim)" % path)
        import importlib.util
        from . import build
        spec = importlib.util.spec_from_file_location("_dmb_torch_shim", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        if mod.build_id() != build.shim_digest():
            raise DmbLibraryError("lib/_dmb_torch_shim.so was not built from the csrc/torch_shim.cpp, dmb_hip.h and torch next to it")
        if mod.library_build_id() != lib.dmb_build_id().decode() or mod.abi_version() != ABI_VERSION:
            raise DmbLibraryError("lib/_dmb_torch_shim.so is bound to another libdmb_hip.so than the one loaded")
        mod.set_error_class(DmbLibraryError)
        _shim, _shim_state = mod, "loaded"
    except Exception as e:  # noqa: BLE001  (any failure to bring the shim up leaves the ctypes binding of the same C ABI)
        _shim, _shim_state = None, "%s: %s" % (type(e).__name__, e)
        if mode == "require":
            raise
    return _shim


def shim_state():
    shim()
    return _shim_state


def check(code, what):
    if code != 0:
        msg = load().dmb_last_error()
        raise DmbLibraryError("%s failed with code %d (%s)" % (what, code, msg.decode() if msg else ""))


def dev_ptr(t, name="tensor", allow_none=False, current=None):
    """Device pointer of a contiguous FP32 HIP tensor; raises for anything else (no silent CPU path).  ``current``: the current
    device's index where the caller has asked for it already (``launch``: once per call, not once per operand)."""
    if t is None:
        if allow_none:
            return None
        raise DmbLibraryError("%s is None" % name)
    if not isinstance(t, torch.Tensor):
        raise DmbLibraryError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise DmbLibraryError(
            "%s lives on %s: the dmb HIP path only runs on a GPU (cuda/hip) tensor and has no CPU fallback" % (name, t.device))
    if t.dtype != torch.float32 and t.dtype != torch.float64 and t.dtype != torch.int64:
        raise DmbLibraryError("%s has dtype %s; FP32 expected" % (name, t.dtype))
    if not t.is_contiguous():
        raise DmbLibraryError("%s must be contiguous" % name)
    if t.device.index != (torch.cuda.current_device() if current is None else current):   # every operand, not only the stream's
        raise DmbLibraryError("%s lives on cuda:%d but the current device is cuda:%d" % (name, t.device.index, torch.cuda.current_device()))
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    """The caller's current HIP stream on ``device``.  Kernels launch on the calling thread's CURRENT device: a tensor that
    lives on another one is refused here instead of failing inside the launch (or worse, on a foreign stream)."""
    if device is not None and getattr(device, "index", None) is not None and device.index != torch.cuda.current_device():
        raise DmbLibraryError("operand on cuda:%d but the current device is cuda:%d: wrap the call in torch.cuda.device(%d) "
                              "(one process per GPU sets it once)" % (device.index, torch.cuda.current_device(), device.index))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def host_ints(values):
    arr = (ctypes.c_int * len(values))(*[int(v) for v in values])
    return arr


def host_floats(values):
    arr = (ctypes.c_float * len(values))(*[float(v) for v in values])
    return arr


# ---------------------------------------------------------------------------------------------- one launch call
class _Absent:
    """``opt(None)``: the NULL a call site passes for an optional operand it leaves out."""

    def __repr__(self):
        return "NULL"


NULL = _Absent()


def opt(operand):
    """Marks an OPTIONAL operand at a ``launch`` call site: None goes to the kernel as NULL.  A bare None is refused there."""
    return NULL if operand is None else operand


def _host_slot(label, array):
    def convert(a):
        if a is NULL:
            return None
        if a is None:
            raise DmbLibraryError("%s is None" % label)
        return a if isinstance(a, ctypes.Array) else array(a)
    return convert


def _slot(ctype, label):
    if ctype is ctypes.c_void_p:
        return None, label      # a device pointer: ``launch`` hands it to dev_ptr under this name
    if ctype in (_HI, _HF):
        return _host_slot(label, host_ints if ctype is _HI else host_floats), label
    return (int if ctype in (ctypes.c_int, ctypes.c_longlong) else float), label


# entry point -> (converter, "entry point: parameter") per argument before `stream`, for the entry points that take one (built once, here)
_LAUNCH = {name: tuple(_slot(t, "%s: %s" % (name, p)) for t, p in params[:-1])
           for name, (_, params) in PROTOTYPES.items() if params and params[-1] == (ctypes.c_void_p, "stream")}


def launch(name, *args, device=None):
    """Enqueue the entry point ``name`` on the current stream: ``args`` are its arguments in the header's order without the stream,
    converted by the header's types --
      a device pointer takes a tensor (``dev_ptr``'s checks, the error names the C parameter) or, untouched, a ctypes pointer or
        array (a channel window of a tensor, a host array of device pointers, a table);
      a ``*_host`` array takes a sequence of numbers (or a ctypes array);
      ``int`` / ``long long`` and ``float`` / ``double`` go through int() and float();
      ``opt(x)`` where the operand may be absent: None is then NULL.  A bare None raises, before anything is launched.
    The stream is the current one of the first tensor's device -- ``dev_ptr`` refuses every operand that is not on the current
    device, so any tensor names the same stream -- or of ``device`` where it is given (no tensor among the operands).  A non-zero
    return code raises DmbLibraryError with the library's last error."""
    slots = _LAUNCH.get(name)
    if slots is None:
        raise DmbLibraryError("%s is not an entry point of include/dmb_hip.h that takes a stream" % name)
    if len(args) != len(slots):
        raise DmbLibraryError("%s takes %d arguments before the stream, got %d" % (name, len(slots), len(args)))
    out, current = [], None
    for (convert, label), a in zip(slots, args):
        if convert is not None:             # int, float, or a host array's converter
            a = convert(a)
        elif a is NULL:
            a = None
        elif not isinstance(a, (ctypes.c_void_p, ctypes.Array)):    # those: a channel window, an array of device pointers, a table
            if current is None and isinstance(a, torch.Tensor) and a.is_cuda:
                current = torch.cuda.current_device()
                if device is None:
                    device = a.device
            a = dev_ptr(a, label, current=current)
        out.append(a)
    if device is None:
        raise DmbLibraryError("%s: no tensor among the operands and no device= to take the stream from" % name)
    check(getattr(load(), name)(*out, stream_ptr(device)), name)
