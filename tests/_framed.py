"""Guarded, poisoned device buffers for the memory-contract tests (tests/test_memory_contract_gpu.py).

``Frame(kind)`` hands out tensors whose storage is the middle of a larger buffer: GUARD bytes of a guard pattern on either side, the
body filled with a second pattern.  ``framed_library(frame)`` makes the package's own allocations (``torch.empty`` / ``empty_like`` /
``zeros`` / ``zeros_like`` in ops.py and the modules) come from the frame, so that a launch's outputs, intermediates and workspaces
start poisoned and sit between guards.  What the tests then read off:

  frame.check()        every guard word of every buffer is intact        -> nothing wrote outside an operand
  frame.unwritten(t)   body-pattern words left in ``t``                   -> every output element was written
  bit-identity with a run on plain tensors                                -> nothing READ a guard or an unwritten body

Two pattern pairs, because a kernel that reads poison must be loud under both: quiet NaNs with distinct payloads ("nan"), and
+-3.0e38f ("huge": ``fmaxf(NaN, 0) == 0``, so a ReLU epilogue swallows a NaN but not a huge value).  Patterns are written as
32-bit words whatever the dtype: FP64 and int64 buffers then hold huge finite values.

Works on CPU tensors as well (tests/test_framed_host.py checks the helper itself there)."""
import contextlib
import struct
import sys
import types

import torch

GUARD = 64 * 1024          # bytes on either side; a multiple of 512, so a body keeps the alignment of the raw allocation


def _i32(bits):
    return bits - (1 << 32) if bits >= 1 << 31 else bits


def _f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


# kind -> (guard word, body word) as int32 values
PATTERNS = {
    "nan": (_i32(0x7FC0BEEF), _i32(0x7FC0DEAD)),
    "huge": (_i32(_f32_bits(3.0e38)), _i32(_f32_bits(-3.0e38))),
}

_ITEMSIZE = {torch.float32: 4, torch.float64: 8, torch.int32: 4, torch.int64: 8, torch.uint8: 1, torch.int8: 1, torch.float16: 2,
             torch.bfloat16: 2, torch.int16: 2, torch.bool: 1}


class _Buf:
    __slots__ = ("raw", "off", "nbytes", "shape", "dtype")

    def __init__(self, raw, off, nbytes, shape, dtype):
        self.raw, self.off, self.nbytes, self.shape, self.dtype = raw, off, nbytes, shape, dtype


class Frame:
    def __init__(self, pass_kind, misalign=0):
        if pass_kind not in PATTERNS:
            raise ValueError("pass kind must be one of %s" % sorted(PATTERNS))
        if misalign % 4 or not 0 <= misalign < 16:
            raise ValueError("misalign must be 0, 4, 8 or 12 bytes")
        self.kind, self.misalign = pass_kind, misalign
        self.guard_word, self.body_word = PATTERNS[pass_kind]
        self.buffers = []      # keeps every raw buffer alive: no block is handed out twice within one frame

    # ------------------------------------------------------------------------------------------ allocation
    def alloc(self, shape, dtype=torch.float32, device="cpu", body="poison", misalign=0):
        """A contiguous ``dtype`` tensor of ``shape`` between two guards.  ``body``: "poison" (the body pattern), "zero", or None
        (left as the guard pattern: the caller overwrites it, see ``input``).  ``misalign``: bytes the body is shifted by -- the
        frame's own value for what a CALLER hands in (``input``, ``out``), 0 for what the library allocates itself (the allocator
        it uses in production never returns a misaligned block)."""
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * _ITEMSIZE[dtype]
        padded = (nbytes + 3) // 4 * 4         # patterns are 32-bit words; a byte tensor's tail shares its last word with the guard
        if _ITEMSIZE[dtype] != 4:
            misalign = 0                       # (a view of a wider dtype cannot start at 4 bytes; byte tensors stay where they are)
        off = GUARD + misalign
        raw = torch.empty((off + padded + GUARD,), dtype=torch.uint8, device=device)
        assert raw.data_ptr() % 16 == 0, "the allocator's blocks are expected to be 16-byte aligned"
        words = raw.view(torch.int32)
        words.fill_(self.guard_word)
        if body == "poison":
            words[off // 4:(off + padded) // 4] = self.body_word
        elif body == "zero":
            words[off // 4:(off + padded) // 4] = 0
        t = raw[off:off + nbytes].view(dtype).view(shape)
        assert t.is_contiguous() and t.data_ptr() % 16 == misalign
        self.buffers.append(_Buf(raw, off, padded, shape, dtype))
        return t

    def input(self, cpu_tensor):
        """A framed device copy of an operand (on the CPU when there is no GPU: the host test)."""
        device = "cuda" if torch.cuda.is_available() else "cpu"
        src = cpu_tensor.detach().contiguous()
        t = self.alloc(src.shape, src.dtype, device, body=None, misalign=self.misalign)
        t.copy_(src)
        return t

    def out(self, shape, dtype=torch.float32, device=None):
        """A caller-owned, poisoned output tensor (``out=`` arguments): everything a wrapper does not write keeps the body pattern."""
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        return self.alloc(shape, dtype, device, "poison", misalign=self.misalign)

    # ------------------------------------------------------------------------------------------ checks
    def check(self):
        """Every guard word of every buffer allocated so far is intact (bitwise, on an int32 view)."""
        if not self.buffers:
            return
        bad = []
        for b in self.buffers:
            w = b.raw.view(torch.int32)
            bad.append((w[:b.off // 4] != self.guard_word).any() | (w[(b.off + b.nbytes) // 4:] != self.guard_word).any())
        flags = torch.stack(bad).cpu()             # one synchronisation for all buffers
        if not bool(flags.any()):
            return
        msgs = []
        for b, f in zip(self.buffers, flags.tolist()):
            if not f:
                continue
            w = b.raw.view(torch.int32).cpu()
            front = (w[:b.off // 4] != self.guard_word).nonzero().flatten()
            back = (w[(b.off + b.nbytes) // 4:] != self.guard_word).nonzero().flatten()
            if front.numel():      # offsets in bytes relative to the body's first byte
                first, n = int(front[0]) * 4 - b.off, int(front.numel())
                msgs.append("%s %s: %d guard words BEFORE the body changed, first at byte offset %d" % (b.shape, b.dtype, n, first))
            if back.numel():
                first, n = b.nbytes + int(back[0]) * 4, int(back.numel())
                msgs.append("%s %s: %d guard words AFTER the body changed, first at byte offset %d (the body ends at %d)"
                            % (b.shape, b.dtype, n, first, b.nbytes))
        raise AssertionError("guard damaged (%s pass): " % self.kind + "; ".join(msgs[:8]))

    def unwritten(self, t):
        """Number of 32-bit words of ``t`` that still hold the body pattern."""
        flat = t.detach().contiguous().view(-1)
        return int((flat.view(torch.int32) == self.body_word).sum().item())


# ---------------------------------------------------------------------------------------------- the library on framed memory
_PACKAGE = "densematchingbenchmark_amd"
# modules that allocate device memory today; every other loaded module of the package that uses ``torch`` is patched as well
_ALLOCATING = ("ops", "modeling.stereo.layers.train_fn", "modeling.stereo.backbones.PSMNet", "modeling.stereo.backbones.AnyNet",
               "modeling.stereo.cmn.cmn", "modeling.stereo.cost_processors.utils.gwc_fms", "modeling.stereo.disp_refinement.utils.edge_aware",
               "modeling.stereo.disp_samplers.DeepPruner", "modeling.stereo.layers.basic_layers", "evaluation.stereo")


def _shape_of(args):
    if len(args) == 1 and not isinstance(args[0], int):
        return tuple(args[0])
    return tuple(args)


def torch_proxy(frame):
    """A module object that is ``torch`` except for the four allocating functions."""
    proxy = types.ModuleType("torch")
    proxy.__dict__["__getattr__"] = lambda name: getattr(torch, name)      # (PEP 562: everything else passes through)

    def _framed(real, body):
        def fn(*size, dtype=None, device=None, requires_grad=False, **other):
            if other or not size:
                return real(*size, dtype=dtype, device=device, requires_grad=requires_grad, **other)
            t = frame.alloc(_shape_of(size), dtype or torch.get_default_dtype(), device if device is not None else "cpu", body)
            return t.requires_grad_() if requires_grad else t
        return fn

    def _framed_like(real, body):
        def fn(t, dtype=None, device=None, requires_grad=False, **other):
            if other or not t.is_contiguous():
                return real(t, dtype=dtype, device=device, requires_grad=requires_grad, **other)
            r = frame.alloc(t.shape, dtype or t.dtype, device if device is not None else t.device, body)
            return r.requires_grad_() if requires_grad else r
        return fn

    proxy.empty, proxy.zeros = _framed(torch.empty, "poison"), _framed(torch.zeros, "zero")
    proxy.empty_like, proxy.zeros_like = _framed_like(torch.empty_like, "poison"), _framed_like(torch.zeros_like, "zero")
    return proxy


@contextlib.contextmanager
def framed_library(frame, shim=False):
    """The package's allocations come from ``frame`` for the duration.  ``shim`` False: the torch-extension shim is off as well (its
    nine entry points allocate in C++, where Python cannot frame them), so every launch goes through the ctypes wrappers."""
    import importlib
    for name in _ALLOCATING:
        importlib.import_module("%s.%s" % (_PACKAGE, name))
    from densematchingbenchmark_amd import _lib, ops
    proxy = torch_proxy(frame)
    patched = []
    _lib.shim()                                   # settle its state first: it is switched off below by hiding the loaded module
    saved_shim, saved_ws = _lib._shim, dict(ops._deconv_ws)
    try:
        for name, mod in list(sys.modules.items()):
            if mod is not None and (name == _PACKAGE or name.startswith(_PACKAGE + ".")) and mod.__dict__.get("torch") is torch:
                mod.torch = proxy
                patched.append(mod)
        if not shim:
            _lib._shim = None
        ops._deconv_ws.clear()                    # the per-stream work-queue workspace is allocated anew, inside the frame
        yield proxy
    finally:
        for mod in patched:
            mod.torch = torch
        _lib._shim = saved_shim
        ops._deconv_ws.clear()
        ops._deconv_ws.update(saved_ws)
