"""The memory contract of every launching wrapper of ``ops``: a call reads and writes exactly its operands.

The value tests compare numbers; none of them sees WHICH memory a launch touches.  Here every wrapper that launches a library kernel
runs on tiny edge shapes three times -- on plain tensors, inside ``framed_library(Frame("nan"))`` and inside
``framed_library(Frame("huge"))`` (tests/_framed.py: operands, outputs, intermediates and workspaces between 64 KiB guards, bodies
poisoned) -- and every framed run must satisfy

  (a) no guard word of any buffer changed;
  (b) every operand is bit-identical to its CPU source afterwards -- except operands a wrapper documents as updated in place
      (``c.put(..., inplace=True)`` below), which must equal the plain run's updated value;
  (c) no returned tensor keeps a word of the body pattern;
  (d) every returned tensor is BIT-identical to the plain run's: no tolerance, so any influence of a guard, of poison or of stale
      memory on a result shows.  One exception: the target-feature gradient of ``fast_fms_bwd`` is summed by LDS atomics in the
      hardware's order (tests/test_head_grads_gpu.py) and is held to that module's rule against FP64 instead;
  (e) a wrapper that writes a window of a caller's tensor (``c.out`` + ``Win``) leaves everything outside the window untouched;
  (f) the entry points of the torch-extension shim that take ``out=`` run once more with the shim ON and a framed ``out``;
  (g) the transposed convolution's work-queue workspace, explicit and "auto", holds zeros after the call (``c.zero_after``).

Cases with ``misalign="ok"`` run a second time with every caller-owned FP32 operand at an address that is only 4-byte aligned (the
dword paths), compared with a plain run on equally misaligned operands; ``misalign="refuse"`` wrappers must raise DmbLibraryError.

Shapes are the smallest at which the edge handling runs: widths with W % 4 in {1, 2, 3} next to 16-byte rows, extents of 1,
B = 2 (the last batch item's end is the operand's end), channel counts off the chunk size, and one shape per kernel family that
spans several tiles / blocks in a partial last one; at most about 2e5 output elements.

The exceptions the table states, all of them:
  (b) updated in place: the tensor of ``zero_columns_``; ``acc`` of ``epe_accumulate`` / ``epe_accumulate_multi``; running mean,
      running variance and ``num_batches_tracked`` of ``bn_train_stats`` / ``bn_train_fwd`` / ``bn_train_act``; the caller's
      work-queue workspace of ``deconv3d_k3s2`` (zeros before, zeros after).  ``dres_acc`` of ``bn_act_bwd`` and the ``residual``
      the data-gradient wrappers take as ``dx_acc`` are READ: the sum lands in the returned tensor, the operand keeps its bits.
  (c) none: no wrapper returns a tensor with padding it leaves unwritten (``deconv3d_k3s2(out_width=)`` returns exactly
      ``out_width`` columns; ``stereo_pad_normalize`` writes its padding; ``patch_match_step(out=)`` writes the range's ends).
  (d) the target-feature gradient of ``fast_fms_bwd``.
  misaligned operands are refused by ``conv3d_k3_x6``, ``conv2d_k3_multi``, ``catconv_first``, ``deconv3d_k3s2`` on row-padded
      input, and by ``conv2d_wgrad`` / ``cat_first_wgrad`` on 16-byte rows; ``conv3d_k3_bnstats`` returns None and launches nothing.
Not framed: what torch itself allocates inside a wrapper (``F.pad``, ``torch.cat``, ``.contiguous()`` copies, ``a + b``) and, with
the shim on, what its C++ side allocates.

Checked by hand when the module was written (not repeated here): ``(i + j) < HW`` widened to ``< HW + 1`` in the scalar epilogue of
csrc/volume.hip failed (a) in every cat_fms / dif_fms case and (e) in cat_fms_into; the zero fill of the group-wise correlation's
VALU form skipped failed (c).  On an MI355X the module takes about 4 s, the slowest case 0.8 s (a first launch)."""
import inspect
import re
import zlib

import pytest
import torch

from oracle import dmb_oracle as O
from tests._framed import PATTERNS, Frame, framed_library

pytestmark = pytest.mark.gpu


class Win:
    """A caller-owned tensor of which only ``index`` (a tuple of slices) belongs to the call."""

    def __init__(self, tensor, index):
        self.tensor, self.index = tensor, index


class AtomicOrder:
    """A result whose summation order is the hardware's: ``truth`` (FP64) and ``ref32`` (the same in FP32) instead of bit-identity."""

    def __init__(self, tensor, truth, ref32):
        self.tensor, self.truth, self.ref32 = tensor, truth, ref32


class Ctx:
    """What a case's body gets: seeded CPU data and the way operands reach the device in this run."""

    def __init__(self, dev, seed, frame=None, misalign=0):
        self.dev, self.frame, self.misalign = dev, frame, misalign
        self.gen = torch.Generator().manual_seed(seed)
        self.operands, self.zeros, self.outs = [], [], 0

    def rand(self, shape, scale=1.0):
        return torch.randn(shape, generator=self.gen) * scale

    def uni(self, shape, lo=0.0, hi=1.0):
        return torch.rand(shape, generator=self.gen) * (hi - lo) + lo

    def _plain(self, shape, dtype):
        if self.misalign and dtype in (torch.float32, torch.int32):
            n = 1
            for s in shape:
                n *= int(s)
            return torch.empty(n + 1, dtype=dtype, device=self.dev)[1:].view(shape)
        return torch.empty(tuple(shape), dtype=dtype, device=self.dev)

    def put(self, cpu, inplace=False):
        cpu = cpu.detach().contiguous()
        if self.frame is not None:
            d = self.frame.input(cpu)
        else:
            d = self._plain(cpu.shape, cpu.dtype)
            d.copy_(cpu)
        self.operands.append((cpu.clone(), d, inplace))
        return d

    def t(self, shape, scale=1.0):
        return self.put(self.rand(shape, scale))

    def affine(self, C):
        return self.put(self.uni((C,), 0.5, 1.5)), self.put(self.uni((C,), -0.5, 0.5))

    def out(self, shape):
        """A caller-owned output, pre-filled with a body pattern (the frame's, or the NaN one on plain memory)."""
        self.outs += 1
        if self.frame is not None:
            return self.frame.out(shape, torch.float32, self.dev)
        d = self._plain(shape, torch.float32)
        d.view(-1).view(torch.int32).fill_(PATTERNS["nan"][1])
        return d

    def zero_after(self, t):
        self.zeros.append(t)
        return t


class Case:
    def __init__(self, wrapper, family, label, body, args, misalign, shim):
        self.wrapper, self.family, self.label, self.body, self.args = wrapper, family, label, body, args
        self.misalign, self.shim = misalign, shim
        self.id = "%s-%s" % (wrapper, label)
        self.seed = zlib.crc32(self.id.encode()) & 0x7FFFFFFF


CASES = {}     # wrapper name -> [Case]
# wrappers that only write into what the caller hands them; every other one allocates an output or a workspace through ops.torch
ALLOCATES_NOTHING = ("zero_columns_", "cat_fms_into", "run_pack_table")


def cases(wrapper, family, calls, misalign="ok", shim=False):
    """Register ``body(ops, c, *args)`` once per entry of ``calls`` ({label: args}) under ``wrapper``."""
    def deco(body):
        for label, args in calls.items():
            CASES.setdefault(wrapper, []).append(Case(wrapper, family, label, body, args if isinstance(args, tuple) else (args,), misalign, shim))
        return body
    return deco


def _ops():
    from densematchingbenchmark_amd import ops
    return ops


def _idx(md, sd=0, dil=1):
    return _ops().disp_index_list(md, sd, dil)


# ================================================================================================ volumes
_VOL = {"w13_b2": ((2, 5, 3, 13), 5, -2, 2), "w24_c32": ((2, 32, 2, 24), 6, 0, 1), "h1_w22": ((1, 3, 1, 22), 4, 0, 1),
        "d_beyond_w": ((1, 4, 2, 5), 9, -1, 1), "w1": ((2, 3, 2, 1), 3, -1, 1), "blocks_w70": ((1, 3, 9, 70), 5, -2, 1)}


@cases("cat_fms", "volumes", _VOL)
def _cat_fms(ops, c, shape, md, sd, dil):
    return [ops.cat_fms(c.t(shape), c.t(shape), _idx(md, sd, dil))]


@cases("dif_fms", "volumes", _VOL)
def _dif_fms(ops, c, shape, md, sd, dil):
    return [ops.dif_fms(c.t(shape), c.t(shape), _idx(md, sd, dil))]


@cases("cat_fms_bwd", "volumes", _VOL)
def _cat_fms_bwd(ops, c, shape, md, sd, dil):
    B, C, H, W = shape
    idx = _idx(md, sd, dil)
    return list(ops.cat_fms_bwd(c.t((B, 2 * C, len(idx), H, W)), idx))


@cases("dif_fms_bwd", "volumes", _VOL)
def _dif_fms_bwd(ops, c, shape, md, sd, dil):
    B, C, H, W = shape
    idx = _idx(md, sd, dil)
    return list(ops.dif_fms_bwd(c.t((B, C, len(idx), H, W)), idx))


@cases("cat_fms_into", "volumes", {"w13_b2": ((2, 5, 3, 13), 5, 3, 2), "w24": ((2, 8, 2, 24), 4, 0, 0), "h1_w22": ((1, 3, 1, 22), 4, 1, 1)})
def _cat_fms_into(ops, c, shape, md, before, after):
    B, C, H, W = shape
    idx = _idx(md)
    out = c.out((B, before + 2 * C + after, len(idx), H, W))
    ops.cat_fms_into(c.t(shape), c.t(shape), idx, out, before)
    return [Win(out, (slice(None), slice(before, before + 2 * C)))]


_FAST = {"w13_b2": ((2, 5, 3, 13), 4), "w24_c32": ((2, 32, 2, 24), 3), "h2_w22": ((1, 3, 2, 22), 5), "blocks_w70": ((1, 4, 5, 70), 6)}


def _fast_ops(c, shape, D, per_pixel=True):
    B, C, H, W = shape
    ds = c.put(c.uni((B, D, H, W), -2.0, 0.6 * W) if per_pixel else torch.linspace(-1.0, W / 2.0, D))
    return c.t(shape), c.t(shape), ds


@cases("fast_cat_fms", "volumes", _FAST)
def _fast_cat(ops, c, shape, D):
    L, R, ds = _fast_ops(c, shape, D)
    L2, R2, lin = _fast_ops(c, shape, D, per_pixel=False)
    return [ops.fast_cat_fms(L, R, ds), ops.fast_cat_fms(L2, R2, lin)]


@cases("fast_dif_fms", "volumes", _FAST)
def _fast_dif(ops, c, shape, D):
    L, R, ds = _fast_ops(c, shape, D)
    return [ops.fast_dif_fms(L, R, ds), ops.fast_dif_fms(L, R, ds, normalize=True, p=1.0), ops.fast_dif_fms(L, R, ds, normalize=True, p=2.0)]


@cases("fast_fms_bwd", "volumes", {"cat_w13_b2": ((2, 5, 3, 13), 4, "cat"), "dif_w24": ((2, 8, 2, 24), 3, "dif"),
                                   "norm_w22": ((1, 3, 2, 22), 5, "norm"), "cat_blocks_w70": ((1, 4, 5, 70), 6, "cat")})
def _fast_bwd(ops, c, shape, D, kind):
    B, C, H, W = shape
    L, R, ds = _fast_ops(c, shape, D)
    a, b, s = (c.operands[-2][0], c.operands[-1][0], c.operands[-3][0])
    if kind == "norm":
        up = c.rand((B, D, H, W))
        nrm = ops.fast_dif_fms(L, R, ds, normalize=True, p=2.0)
        dl, dr, dsamp = ops.fast_fms_bwd(L, R, ds, c.put(up), dif=True, norm_out=nrm, p=2.0, wrt_samples=True)
        kw = dict(kind="dif", normalize=True, p=2.0)
    else:
        up = c.rand((B, 2 * C if kind == "cat" else C, D, H, W))
        dl, dr, dsamp = ops.fast_fms_bwd(L, R, ds, c.put(up), dif=kind == "dif", wrt_samples=True)
        kw = dict(kind=kind)
    t64 = O.fast_volume_grads(a, b, up, disp_sample=s, dtype=torch.float64, wrt_samples=True, **kw)
    t32 = O.fast_volume_grads(a, b, up, disp_sample=s, dtype=torch.float32, wrt_samples=True, **kw)
    return [dl, AtomicOrder(dr, t64[1], t32[1]), dsamp]


_GWC = {"w13_b2": ((2, 12, 3, 13), 3, 5, 0, 1), "w24_mfma": ((2, 16, 2, 24), 2, 6, 0, 1), "h1_w22_neg": ((1, 8, 1, 22), 8, 4, -3, 2),
        "blocks_w70_neg": ((1, 8, 5, 70), 2, 9, -3, 1)}


@cases("gwc_fms", "volumes", _GWC)
def _gwc(ops, c, shape, G, md, sd, dil):
    B, C, H, W = shape
    idx = _idx(md, sd, dil)
    out = c.out((B, G + 3, len(idx), H, W))
    ops.gwc_fms(c.t(shape), c.t(shape), idx, G, out=out, out_ch_offset=2)
    return [ops.gwc_fms(c.t(shape), c.t(shape), idx, G), Win(out, (slice(None), slice(2, 2 + G)))]


@cases("correlation1d", "volumes", {"w13_b2": ((2, 5, 3, 13), 6), "w24_c32": ((2, 32, 2, 24), 9), "h1_w22": ((1, 3, 1, 22), 33),
                                    "blocks_w70": ((1, 4, 5, 70), 12)})
def _corr(ops, c, shape, D):
    return [ops.correlation1d(c.t(shape), c.t(shape), D)]


# ================================================================================================ 3-D convolutions
def _w3(c, Co, Ci, transposed=False):
    return c.t((Ci, Co, 3, 3, 3) if transposed else (Co, Ci, 3, 3, 3), 1.0 / (Ci * 27) ** 0.5)


@cases("pack_conv3d_weights", "conv3d_s1", {"5to32": (32, 5), "33to64": (64, 33), "64to128": (128, 64)})
def _pack3(ops, c, Co, Ci):
    return [ops.pack_conv3d_weights(_w3(c, Co, Ci))]


@cases("pack_deconv3d_weights", "deconv3d", {"33to32": (32, 33), "64to64": (64, 64), "5to1": (1, 5), "16to7": (7, 16)})
def _packd(ops, c, Co, Ci):
    return [ops.pack_deconv3d_weights(_w3(c, Co, Ci, True))]


@cases("pack_conv3d_dgrad_weights", "gradients", {"32from5": (32, 5), "64from33": (64, 33), "32from64": (32, 64)})
def _packg(ops, c, Co, Ci):
    return [ops.pack_conv3d_dgrad_weights(_w3(c, Co, Ci))]


@cases("pack_conv3d_x6_weights", "conv3d_x6", {"32to32": (32, 32), "5to32": (32, 5), "64to64": (64, 64)})
def _packx6(ops, c, Co, Ci):
    return [ops.pack_conv3d_x6_weights(_w3(c, Co, Ci))]


_S1 = {"w13_b2_ci5": ((2, 5, 3, 5, 13), 32, True, True), "w24_ci32_co64": ((2, 32, 2, 3, 24), 64, "pre", True),
       "d1h1_w22_ci33": ((1, 33, 1, 1, 22), 32, False, False), "w1_co128": ((1, 8, 2, 3, 1), 128, True, False),
       "w48_ci64": ((1, 64, 2, 2, 48), 32, True, True), "tiles_h17_w70": ((1, 8, 3, 17, 70), 32, True, True)}


def _conv3d_unit(ops, c, shape, Co, relu, use_res, stride):
    B, Ci, D, H, W = shape
    wp = ops.pack_conv3d_weights(_w3(c, Co, Ci))
    sc, sh = c.affine(Co)
    oshape = (B, Co) + tuple((e - 1) // stride + 1 for e in (D, H, W))
    res = c.t(oshape) if use_res else None
    out = c.out(oshape)
    x = c.t(shape)
    y = ops.conv3d_k3(x, wp, Co, sc, sh, res, stride, relu)
    ops.conv3d_k3(x, wp, Co, sc, sh, res, stride, relu, out=out)
    return [y, out]


@cases("conv3d_k3", "conv3d_s1", _S1, shim=True)
def _conv3d_s1(ops, c, shape, Co, relu, use_res):
    return _conv3d_unit(ops, c, shape, Co, relu, use_res, 1)


@cases("conv3d_k3", "conv3d_s2", {"s2_w13_b2_ci5": ((2, 5, 3, 5, 13), 32, True, True), "s2_w24_ci32": ((2, 32, 4, 3, 24), 64, "pre", True),
                                  "s2_d1h1_w22_ci33": ((1, 33, 1, 1, 22), 64, False, False), "s2_w48_ci64": ((1, 64, 2, 4, 48), 64, True, True),
                                  "s2_tiles_h17_w70": ((1, 16, 5, 17, 70), 64, True, True)},
       shim=True)
def _conv3d_s2(ops, c, shape, Co, relu, use_res):
    return _conv3d_unit(ops, c, shape, Co, relu, use_res, 2)


@cases("conv3d_k3_x6", "conv3d_x6", {"w48_co32_b2": ((2, 32, 2, 3, 48), 32, True), "w24_co64_ci5": ((2, 5, 1, 2, 24), 64, False),
                                     "w96_d1h1": ((1, 32, 1, 1, 96), 32, True), "tiles_h17_w48": ((1, 32, 3, 17, 48), 32, True)}, misalign="refuse")
def _x6(ops, c, shape, Co, use_res):
    B, Ci, D, H, W = shape
    wp = ops.pack_conv3d_x6_weights(_w3(c, Co, Ci))
    sc, sh = c.affine(Co)
    return [ops.conv3d_k3_x6(c.t(shape), wp, Co, sc, sh, c.t((B, Co, D, H, W)) if use_res else None, True)]


@cases("conv3d_k3_c1", "conv3d_c1", {"w13_b2_ci5": ((2, 5, 3, 4, 13), True), "w24_ci32": ((2, 32, 2, 3, 24), False),
                                     "d1h1_w22": ((1, 2, 1, 1, 22), True), "w64_ci32": ((1, 32, 3, 2, 64), True),
                                     "tiles_h19_w130": ((1, 5, 4, 19, 130), True)})
def _c1(ops, c, shape, use_res):
    B, Ci, D, H, W = shape
    return [ops.conv3d_k3_c1(c.t(shape), _w3(c, 1, Ci), 0.25, c.t((B, 1, D, H, W)) if use_res else None)]


_DECONV = {"w13_b2_ci9": ((2, 9, 2, 3, 13), 64, True, True, "auto"), "w24_ci64_ws": ((2, 64, 2, 2, 24), 32, "pre", True, "own"),
           "d1h1_w5_co7": ((1, 16, 1, 1, 5), 7, False, False, None), "w12_ci32_co64_ws": ((2, 32, 1, 3, 12), 64, True, True, "auto"),
           "w1_co1": ((1, 5, 2, 2, 1), 1, False, False, "auto"), "tiles_h7_w35": ((1, 32, 3, 7, 35), 32, True, True, "auto"),
           "tiles_h7_w36_ws": ((1, 32, 3, 7, 36), 64, True, True, "auto")}


@cases("deconv3d_k3s2", "deconv3d", _DECONV, shim=True)
def _deconv(ops, c, shape, Co, relu, use_res, ws):
    from densematchingbenchmark_amd import _lib
    B, Ci, D, H, W = shape
    wp = ops.pack_deconv3d_weights(_w3(c, Co, Ci, True))
    sc, sh = c.affine(Co)
    oshape = (B, Co, 2 * D, 2 * H, 2 * W)
    res = c.t(oshape) if use_res else None
    x = c.t(shape)
    if ws == "own":      # the caller's workspace: zeros before (torch.zeros inside ops is framed, this one is an operand) and after
        ws = c.zero_after(c.put(torch.zeros(_lib.DECONV3D_WORKSPACE_BYTES // 4, dtype=torch.int32), inplace=True))
    out = c.out(oshape)
    y = ops.deconv3d_k3s2(x, wp, Co, sc, sh, res, relu, workspace=ws)
    ops.deconv3d_k3s2(x, wp, Co, sc, sh, res, relu, workspace=ws, out=out)
    if isinstance(ws, str):
        c.zero_after(ops.deconv3d_workspace(x.device))
    return [y, out]


@cases("deconv3d_k3s2", "deconv3d", {"padded_rows_w6": ((2, 32, 1, 2, 6), 32), "padded_rows_w14_co64": ((1, 64, 2, 1, 14), 64)}, misalign="refuse")
def _deconv_padded(ops, c, shape, Co):
    """Rows zero-padded to a multiple of 4 columns, ``out_width`` = 2 x the real width (ops.deconv3d_k3s2 docstring): the output has
    exactly ``out_width`` columns, so nothing of it is padding."""
    B, Ci, D, H, W = shape
    Wp = (W + 3) // 4 * 4
    x = torch.zeros((B, Ci, D, H, Wp))
    x[..., :W] = c.rand(shape)
    wp = ops.pack_deconv3d_weights(_w3(c, Co, Ci, True))
    y = ops.deconv3d_k3s2(c.put(x), wp, Co, None, None, c.t((B, Co, 2 * D, 2 * H, 2 * W)), True, out_width=2 * W)
    c.zero_after(ops.deconv3d_workspace(y.device))
    return [y]


@cases("copy_window", "catconv", {"w13_left": ((2, 3, 2, 13), 8, 0), "w24_shift": ((2, 4, 3, 24), 28, -4), "w22_tail": ((1, 5, 1, 22), 12, 10),
                                  "pad_to_4": ((1, 2, 2, 2, 6), 8, 0), "rows_w70": ((1, 2, 9, 70), 72, -1)})
def _copy_window(ops, c, shape, Wd, xs):
    return [ops.copy_window(c.t(shape), Wd, xs)]


@cases("zero_columns_", "catconv", {"w8_from6": ((2, 3, 2, 2, 8), 6), "w16_from13": ((1, 2, 1, 3, 16), 13), "w5_from0": ((2, 2, 3, 5), 0),
                                    "w8_none": ((1, 2, 2, 8), 8)})
def _zero_columns(ops, c, shape, x0):
    t = c.put(c.rand(shape), inplace=True)          # updated in place (ops.zero_columns_: "t[..., x0:] = 0 in place")
    assert ops.zero_columns_(t, x0) is t
    return [t]


_CATCONV = {"b2_c5_d4_w12": (2, 5, 32, 4, 3, 12, "cat"), "c32_d8_w24": (2, 32, 32, 8, 2, 24, "dif"), "h1_co16_d4_w16": (1, 8, 16, 4, 1, 16, "cat"),
            "tiles_d8_h9_w72": (1, 8, 32, 8, 9, 72, "cat")}


@cases("catconv_pack", "catconv", {"cat_c5_co32": (32, 5, "cat"), "dif_c33_co8": (8, 33, "dif"), "cat_c32_co32": (32, 32, "cat")})
def _catconv_pack(ops, c, Co, C, kind):
    p = ops.catconv_pack(c.t((Co, C if kind == "dif" else 2 * C, 3, 3, 3)), kind)
    return [p[k] for k in ("A", "B1", "B2", "HC", "HD")]


@cases("catconv_first", "catconv", _CATCONV, misalign="refuse")
def _catconv_first(ops, c, B, C, Co, D, H, W, kind):
    Cin = C if kind == "dif" else 2 * C
    packs = ops.catconv_pack(c.t((Co, Cin, 3, 3, 3), 1.0 / (Cin * 27) ** 0.5), kind)
    sc, sh = c.affine(Co)
    L, R = c.t((B, C, H, W)), c.t((B, C, H, W))
    assert ops.catconv_applicable(L, R, list(range(D)), Co)
    return [ops.catconv_first(L, R, D, packs, sc, sh, True)]


def _cat_first_wgrad(ops, c, B, C, Co, D, H, W, kind):
    return [ops.cat_first_wgrad(c.t((B, C, H, W)), c.t((B, C, H, W)), c.t((B, Co, D, H, W)), kind)]


# (the 2-D weight gradient stages 16-byte units: rows that are no multiple of 4 columns are zero-padded into fresh tensors by
# ops.conv2d_wgrad, so misaligned operands are fine there; 16-byte rows go to the kernel as they are and it refuses a misaligned base)
cases("cat_first_wgrad", "catconv", _CATCONV, misalign="refuse")(_cat_first_wgrad)
cases("cat_first_wgrad", "catconv", {"w13_c3_d3": (2, 3, 8, 3, 2, 13, "cat"), "h1_w22_dif": (1, 5, 4, 2, 1, 22, "dif")})(_cat_first_wgrad)


@cases("conv2d_k3_multi", "catconv", {"two_widths_b2": (2, 5, 32, 3, (12, 8)), "three_jobs_ci32": (1, 32, 64, 2, (24, 24, 4)),
                                      "h1": (2, 3, 128, 1, (16,))}, misalign="refuse")
def _conv2d_multi(ops, c, B, Ci, Co, H, widths):
    jobs, res = [], []
    for q, W in enumerate(widths):
        out = c.out((B, Co + 8, H, W))
        wp = ops.pack_conv2d_weights(c.t((Co, Ci, 3, 3), 1.0 / (Ci * 9) ** 0.5))
        jobs.append((c.t((B, Ci, H, W)), wp, out, 8 if q % 2 else 0))
        res.append(Win(out, (slice(None), slice(8, Co + 8) if q % 2 else slice(0, Co))))
    ops.conv2d_k3_multi(jobs, Co)
    return res


# ================================================================================================ 2-D convolutions and resamplers
@cases("pack_conv2d_weights", "conv2d", {"k3_5to32": (32, 5, 3), "k1_33to128": (128, 33, 1), "k5_3to32": (32, 3, 5), "k3_64to1": (1, 64, 3)})
def _pack2(ops, c, Co, Ci, k):
    return [ops.pack_conv2d_weights(c.t((Co, Ci, k, k)))]


_C2D = {"k3_w13_b2_ci5": ((2, 5, 7, 13), 32, 3, 1, 1, True), "k3_w24_ci32_co64": ((2, 32, 5, 24), 64, 3, 1, 2, True),
        "k1_h1_w22_ci33_co128": ((1, 33, 1, 22), 128, 1, 1, 1, False), "k3s2_w13": ((2, 3, 9, 13), 32, 3, 2, 1, True),
        "k5s2_w48": ((1, 3, 6, 48), 32, 5, 2, 1, False), "k3_co1_w5": ((2, 20, 3, 5), 1, 3, 1, 1, True),
        "dil4_w22": ((1, 8, 9, 22), 32, 3, 1, 4, False), "w1": ((2, 4, 3, 1), 64, 3, 1, 1, True),
        "k3_tiles_h20_w100": ((1, 8, 20, 100), 64, 3, 1, 1, True), "k3s2_tiles_h33_w101": ((1, 16, 33, 101), 32, 3, 2, 1, True)}


@cases("conv2d", "conv2d", _C2D, shim=True)
def _conv2d(ops, c, shape, Co, k, stride, dil, use_res):
    B, Ci, H, W = shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    wp = ops.pack_conv2d_weights(c.t((Co, Ci, k, k), 1.0 / (Ci * k * k) ** 0.5))
    sc, sh = c.affine(Co)
    x = c.t((B, Ci + 3, H, W))                                        # read through a channel window
    res = c.t((B, Co + 2, Ho, Wo)) if use_res else None
    out = c.out((B, Co + 5, Ho, Wo))
    y = ops.conv2d(x, wp, Co, k, stride, dil, sc, sh, res, True, in_window=(3, Ci), res_ch_offset=2)
    ops.conv2d(x, wp, Co, k, stride, dil, sc, sh, res, True, in_window=(3, Ci), out=out, out_ch_offset=4, res_ch_offset=2)
    return [y, Win(out, (slice(None), slice(4, 4 + Co)))]


@cases("conv2d_dgrad", "gradients", {"k3_w13_ci5": ((2, 32, 4, 13), 5, 3, 1), "k3_w24_ci130": ((2, 32, 2, 24), 130, 3, 1),
                                     "k1_h1_w22_ci80": ((1, 16, 1, 22), 80, 1, 1)})
def _conv2d_dgrad(ops, c, dshape, Ci, k, dil):
    B, Co, H, W = dshape
    return [ops.conv2d_dgrad(c.t(dshape), c.t((Co, Ci, k, k)), dil, residual=c.t((B, Ci, H, W)))]


def _conv2d_wgrad(ops, c, shape, Co, k, dil):
    B, Ci, H, W = shape
    return [ops.conv2d_wgrad(c.t(shape), c.t((B, Co, H, W)), k, dil)]


cases("conv2d_wgrad", "gradients", {"k3_w13_b2": ((2, 5, 4, 13), 32, 3, 1), "k1_h1_w22": ((1, 33, 1, 22), 64, 1, 1)})(_conv2d_wgrad)
cases("conv2d_wgrad", "gradients", {"k3_w24_dil2": ((2, 32, 3, 24), 33, 3, 2), "k3_w48_b2": ((2, 5, 2, 48), 128, 3, 1)}, misalign="refuse")(_conv2d_wgrad)


@cases("avgpool2d", "conv2d", {"k2_w13_b2": ((2, 5, 6, 13), 2, None), "k4_w24_window": ((2, 6, 8, 24), 4, (1, 3)), "k8_one_out": ((1, 3, 8, 8), 8, None)})
def _avgpool(ops, c, shape, k, window):
    return [ops.avgpool2d(c.t(shape), k, window)]


@cases("avgpool2d_bwd", "conv2d", {"k2_w13_b2": ((2, 5, 3, 6), (6, 13), 2), "k4_w24": ((2, 3, 2, 6), (8, 24), 4), "k8_one_in": ((1, 3, 1, 1), (8, 8), 8)})
def _avgpool_bwd(ops, c, gshape, in_hw, k):
    return [ops.avgpool2d_bwd(c.t(gshape), in_hw, k)]


_RESIZE = {"w13_b2": ((2, 3, 3, 5), (7, 13)), "w24": ((2, 4, 4, 8), (8, 24)), "from_1x1_to_w22": ((1, 2, 1, 1), (3, 22)), "to_1x1": ((1, 2, 3, 5), (1, 1)),
           "blocks_w70": ((1, 2, 9, 20), (31, 70))}


@cases("bilinear_ac", "conv2d", _RESIZE)
def _bilinear_ac(ops, c, shape, out_hw):
    B, C = shape[:2]
    out = c.out((B, C + 3, *out_hw))
    ops.bilinear_ac(c.t(shape), out_hw, out=out, out_ch_offset=2)
    return [ops.bilinear_ac(c.t(shape), out_hw), Win(out, (slice(None), slice(2, 2 + C)))]


@cases("bilinear_scale", "conv2d", _RESIZE)
def _bilinear_scale(ops, c, shape, out_hw):
    B, C = shape[:2]
    out = c.out((B, C + 3, *out_hw))
    ops.bilinear_scale(c.t(shape), out_hw, 2.5, out=out, out_ch_offset=1)
    return [ops.bilinear_scale(c.t(shape), out_hw, 2.5), Win(out, (slice(None), slice(1, 1 + C)))]


@cases("bilinear_ac_bwd", "conv2d", _RESIZE)
def _bilinear_ac_bwd(ops, c, shape, out_hw):
    return [ops.bilinear_ac_bwd(c.t(shape[:2] + tuple(out_hw)), shape[2:])]


@cases("bilinear_scale_bwd", "conv2d", _RESIZE)
def _bilinear_scale_bwd(ops, c, shape, out_hw):
    return [ops.bilinear_scale_bwd(c.t(shape[:2] + tuple(out_hw)), shape[2:], 2.5)]


# ================================================================================================ regression ends
def _vals(D):
    return _ops().disp_sample_values(D, 0, 1)


_COST = {"w13_b2": (2, 5, 3, 13), "w24_d24": (2, 24, 2, 24), "h1_w22": (1, 7, 1, 22), "d1_w5": (1, 1, 2, 5), "w1": (2, 3, 2, 1), "blocks_w70": (1, 12, 9, 70)}


@cases("soft_argmin", "regression", _COST)
def _soft_argmin(ops, c, *shape):
    cost = c.t(shape, 3.0)
    return [ops.soft_argmin(cost, _vals(shape[1]), 1.0, True), ops.soft_argmin(cost, _vals(shape[1]), 0.5, False)]


@cases("soft_argmin_sampled", "regression", _COST)
def _soft_argmin_sampled(ops, c, *shape):
    return [ops.soft_argmin_sampled(c.t(shape, 3.0), c.t(shape, 10.0), 1.0, True)]


@cases("soft_argmin_bwd", "regression", _COST)
def _soft_argmin_bwd(ops, c, *shape):
    B, D, H, W = shape
    cost = c.t(shape, 3.0)
    disp = ops.soft_argmin(cost, _vals(D), 1.0, True)
    return [ops.soft_argmin_bwd(cost, disp, c.t((B, 1, H, W)), _vals(D), 1.0)]


@cases("local_soft_argmin", "regression", {"w13_b2_r2": ((2, 12, 3, 13), 2, 1), "w24_r3_rd2": ((2, 24, 2, 24), 3, 2), "h1_w22_r0": ((1, 7, 1, 22), 0, 1)})
def _local_soft_argmin(ops, c, shape, radius, rd):
    cost = c.t(shape, 4.0)
    return list(ops.local_soft_argmin(cost, radius, rd, 0, 1, 1.0, return_index=True)) + [ops.local_soft_argmin(cost, radius, rd, -4, 2, 1.0)]


_TRI = {"w13_b2": ((2, 3, 4, 5), (9, 13, 13)), "w24_x4": ((2, 4, 3, 6), (16, 12, 24)), "in1_w22": ((1, 1, 1, 1), (4, 3, 22)),
        "out1": ((1, 3, 2, 5), (5, 1, 1)), "blocks_w70": ((1, 5, 6, 20), (17, 21, 70))}


@cases("trilinear_ac", "regression", _TRI)
def _trilinear(ops, c, ins, outs):
    return [ops.trilinear_ac(c.t(ins), outs)]


@cases("trilinear_ac_bwd", "regression", _TRI)
def _trilinear_bwd(ops, c, ins, outs):
    return [ops.trilinear_ac_bwd(c.t(ins[:1] + tuple(outs)), ins[1:])]


@cases("trilinear_soft_argmin", "regression", _TRI)
def _trilinear_sa(ops, c, ins, outs):
    return [ops.trilinear_soft_argmin(c.t(ins, 3.0), outs, _vals(outs[0]), 1.0)]


@cases("trilinear_ac_soft_argmin", "regression", _TRI)
def _trilinear_ac_sa(ops, c, ins, outs):
    return list(ops.trilinear_ac_soft_argmin(c.t(ins, 3.0), outs, _vals(outs[0]), 1.0))


@cases("trilinear_ac_soft_argmin_bwd", "regression", _TRI)
def _trilinear_ac_sa_bwd(ops, c, ins, outs):
    x = c.t(ins, 3.0)
    B = ins[0]
    _, disp = ops.trilinear_ac_soft_argmin(x, outs, _vals(outs[0]), 1.0)
    g = c.t((B, 1) + tuple(outs[1:]))
    return [ops.trilinear_ac_soft_argmin_bwd(x, disp, g, outs, _vals(outs[0]), 1.0),
            ops.trilinear_ac_soft_argmin_bwd(x, disp, g, outs, _vals(outs[0]), 1.0, grad_cost=c.t((B,) + tuple(outs)))]


_K8 = {"w5_b2": (2, 3, 2, 5), "w6": (2, 6, 3, 6), "h1_w13": (1, 2, 1, 13), "d1_w1": (1, 1, 2, 1), "blocks_w20": (1, 3, 5, 20)}


@cases("deconv3d_k8s4_c1", "regression", _K8)
def _k8s4(ops, c, *shape):
    return [ops.deconv3d_k8s4_c1(c.t(shape), c.t((8, 8, 8), 0.2))]


@cases("deconv3d_k8s4_c1_soft_argmin", "regression", _K8)
def _k8s4_sa(ops, c, *shape):
    x, w = c.t(shape), c.t((8, 8, 8), 0.2)
    return list(ops.deconv3d_k8s4_c1_soft_argmin(x, w, _vals(4 * shape[1]), 1.0)) + [ops.deconv3d_k8s4_c1_soft_argmin(x, w)[0]]


@cases("deconv3d_k8s4_c1_bwd", "regression", _K8)
def _k8s4_bwd(ops, c, *shape):
    B, D, H, W = shape
    x, w, dy = c.t(shape), c.t((8, 8, 8), 0.2), c.t((B, 4 * D, 4 * H, 4 * W))
    return list(ops.deconv3d_k8s4_c1_bwd(x, w, dy)) + [ops.deconv3d_k8s4_c1_bwd(x, w, dy, want_dw=False)[0], ops.deconv3d_k8s4_c1_bwd(x, w, dy, want_dx=False)[1]]


# ================================================================================================ confidence head
@cases("pack_conf_head_weights", "confhead", {"d20_cm6": (6, 20), "d48_cm16": (16, 48), "d12_cm64": (64, 12)})
def _pack_conf(ops, c, Cm, D):
    return [ops.pack_conf_head_weights(c.t((Cm, D, 3, 3)))]


@cases("conf_head", "confhead", {"w13_b2_d20_cm6": ((2, 20, 3, 13), 6), "w24_d48_cm16": ((2, 48, 2, 24), 16), "h1_w22_d12_cm64": ((1, 12, 1, 22), 64),
                                 "tiles_h11_w70": ((1, 20, 11, 70), 16)})
def _conf_head(ops, c, shape, Cm):
    D = shape[1]
    wp = ops.pack_conf_head_weights(c.t((Cm, D, 3, 3), 1.0 / (D * 9) ** 0.5))
    sc, sh = c.affine(Cm)
    return [ops.conf_head(c.t(shape), wp, sc, sh, c.t((Cm,), 0.5))]


@cases("conf_head_from_source", "confhead", {"wq8_b2": (2, 3, 2, 8, True), "wq4_hidden": (2, 2, 3, 4, False), "hq1_wq12": (1, 2, 1, 12, True)})
def _conf_from_source(ops, c, B, Dq, Hq, Wq, dot):
    M = 64
    cq, w8 = c.t((B, Dq, Hq, Wq)), c.t((1, 1, 8, 8, 8), 0.2)
    w1, w2 = c.t((M, 4 * Dq, 3, 3), 1.0 / (Dq * 9) ** 0.5), c.t((M,), 0.3)
    sc, sh = c.affine(M)
    cost = ops.deconv3d_k8s4_c1(cq, w8.view(8, 8, 8))
    ops.UpsampleSource.attach(cost, cq, w8)
    assert ops.conf_head_composite_applicable(cost, M)
    comp = ops.conf_head_k8s4_pack(w1, w8, sc, sh)
    ops.set_conf_dot_epilogue(dot)
    try:
        return [ops.conf_head_from_source(cost, comp, sc, sh, w2)]
    finally:
        ops.set_conf_dot_epilogue(True)


@cases("channel_dot", "confhead", {"s39_b2_c5": (2, 5, (3, 13)), "s48_c64": (2, 64, (2, 24)), "s1": (1, 3, (1, 1)), "s3d": (2, 4, (2, 3, 6))})
def _channel_dot(ops, c, B, C, sp):
    return [ops.channel_dot(c.t((B, C) + sp), c.t((B, 1) + sp))]


# ================================================================================================ losses
_LOSS = {"w13_b2": (2, 6, 3, 13), "w24": (2, 24, 2, 24), "h1_w22": (1, 5, 1, 22), "one_pixel": (1, 4, 1, 1), "blocks_w70": (1, 12, 9, 70)}


def _focal(ops, c, shape, vmap):
    B, D, H, W = shape
    cost = c.t(shape, 2.0)
    gt = c.put(c.uni((B, 1, H, W), -2.0, D + 2.0))
    var = c.put(c.uni((B, 1, H, W), 0.5, 2.0)) if vmap else 1.2
    return cost, gt, var, [float(v) for v in range(D)], (0, D, 0, D - 1, 5.0)


@cases("stereo_focal_loss_fwd", "losses", _LOSS)
def _focal_fwd(ops, c, *shape):
    res = []
    for vmap in (False, True):
        cost, gt, var, vals, rest = _focal(ops, c, shape, vmap)
        res += list(ops.stereo_focal_loss_fwd(cost, gt, var, vals, *rest))
    return res


@cases("stereo_focal_loss_bwd", "losses", _LOSS)
def _focal_bwd(ops, c, *shape):
    res = []
    for vmap in (False, True):
        cost, gt, var, vals, rest = _focal(ops, c, shape, vmap)
        out, stats = ops.stereo_focal_loss_fwd(cost, gt, var, vals, *rest)
        res += list(ops.stereo_focal_loss_bwd(cost, gt, var, vals, stats, out, c.put(torch.tensor(0.7)), *rest, True))
    return res


_MAP = {"n78_b2": (2, 1, 3, 13), "n96": (2, 1, 2, 24), "n22": (1, 1, 1, 22), "n1": (1, 1, 1, 1), "n4100": (1, 1, 41, 100)}


@cases("map_loss_fwd", "losses", _MAP)
def _map_fwd(ops, c, *shape):
    x, gt = c.t(shape, 3.0), c.put(c.uni(shape, -2.0, 12.0))
    return [ops.map_loss_fwd(x, gt, 0, 10, 0), ops.map_loss_fwd(x, gt, 0, 10, 1)]


@cases("map_loss_bwd", "losses", _MAP)
def _map_bwd(ops, c, *shape):
    x, gt, go = c.t(shape, 3.0), c.put(c.uni(shape, -2.0, 12.0)), c.put(torch.tensor(1.3))
    return [ops.map_loss_bwd(x, gt, ops.map_loss_fwd(x, gt, 0, 10, m), go, 0, 10, m) for m in (0, 1)]


# ================================================================================================ BatchNorm
_BN = {"s195_b2_c5": (2, 5, 3, 5, 13), "s144_c32": (2, 32, 2, 3, 24), "s1_c3": (1, 3, 1, 1, 1), "2d_s22_c33": (2, 33, 1, 22), "blocks_s1260": (2, 8, 4, 9, 35)}


def _running(c, C):
    """Running statistics and the step counter: updated in place (ops.bn_train_fwd docstring)."""
    return (c.put(c.rand((C,), 0.1), inplace=True), c.put(c.uni((C,), 0.5, 1.5), inplace=True),
            c.put(torch.tensor(3, dtype=torch.int64), inplace=True))


@cases("bn_train_stats", "batchnorm", _BN)
def _bn_stats(ops, c, *shape):
    C = shape[1]
    g, b = c.affine(C)
    rm, rv, _ = _running(c, C)
    x = c.t(shape)
    return list(ops.bn_train_stats(x, g, b, rm, rv)) + list(ops.bn_train_stats(x)) + [rm, rv]


@cases("bn_act", "batchnorm", _BN)
def _bn_act(ops, c, *shape):
    sc, sh = c.affine(shape[1])
    x = c.t(shape)
    return [ops.bn_act(x, sc, sh, c.t(shape), True), ops.bn_act(x, sc, sh, c.t(shape), "pre"), ops.bn_act(x, sc, sh)]


@cases("bn_train_fwd", "batchnorm", _BN)
def _bn_fwd(ops, c, *shape):
    C = shape[1]
    g, b = c.affine(C)
    rm, rv, nbt = _running(c, C)
    x = c.t(shape)
    return list(ops.bn_train_fwd(x, g, b, rm, rv, nbt, 0.1, 1e-5, c.t(shape), True)) + list(ops.bn_train_fwd(x)) + [rm, rv, nbt]


@cases("bn_act_bwd", "batchnorm", _BN)
def _bn_bwd(ops, c, *shape):
    C = shape[1]
    g, b = c.affine(C)
    x, dy = c.t(shape), c.t(shape)
    y, mean, invstd, sc, sh = ops.bn_train_fwd(x, g, b, None, None, None, 0.1, 1e-5, c.t(shape), True)
    acc = c.t(shape)      # dres_acc: read, and added into the returned dres (not written: ops.bn_act_bwd docstring)
    res = list(ops.bn_act_bwd(dy, x, y, sc, sh, mean, invstd, True, True, dres_acc=acc))
    res += list(ops.bn_act_bwd(dy, x, None, sc, sh, mean, invstd, False, False, want_dres=True))
    res += list(ops.bn_act_bwd(dy, x, None, sc, sh, mean, invstd, "pre", True))[:3]
    return res


_BNSTATS = {"w48_b2": (2, 32, 2, 3, 48), "w24_ci16": (2, 16, 3, 2, 24), "w60_ci64_d1": (1, 64, 1, 2, 60)}


@cases("conv3d_k3_bnstats", "batchnorm", _BNSTATS, misalign="declines")
def _bnstats(ops, c, *shape):
    fused = ops.conv3d_k3_bnstats(c.t(shape), ops.pack_conv3d_weights(_w3(c, 32, shape[1])), 32)
    assert fused is not None or c.misalign, "the epilogue form is expected to cover this shape"
    return None if fused is None else list(fused)


@cases("conv3d_k3_bnstats", "batchnorm", {"w13_not_covered": (2, 5, 2, 3, 13)}, misalign="declines")
def _bnstats_uncovered(ops, c, *shape):
    assert ops.conv3d_k3_bnstats(c.t(shape), ops.pack_conv3d_weights(_w3(c, 32, shape[1])), 32) is None      # launches nothing
    return []


@cases("bn_train_act", "batchnorm", _BNSTATS)
def _bn_train_act(ops, c, *shape):
    B, Ci, D, H, W = shape
    x = c.t(shape)
    wp = ops.pack_conv3d_weights(_w3(c, 32, Ci))
    before = ops.split_k()
    ops.set_split_k(False)
    try:
        raw = ops.conv3d_k3(x, wp, 32)
    finally:
        ops.set_split_k(before)
    r64 = raw.double()
    parts = torch.stack([r64.sum(dim=(0, 2, 3, 4)), (r64 * r64).sum(dim=(0, 2, 3, 4))], -1).unsqueeze(1)
    parts = c.put(torch.cat([parts.cpu() * 0.25, parts.cpu() * 0.75], 1))            # [C, 2, 2] float64
    g, b = c.affine(32)
    rm, rv, nbt = _running(c, 32)
    return list(ops.bn_train_act(raw, parts, g, b, rm, rv, nbt, 0.1, 1e-5, c.t((B, 32, D, H, W)), True)) + [rm, rv, nbt]


# ================================================================================================ weight and data gradients
@cases("run_pack_table", "gradients", {"s1_64x32": (64, 32, False, 1), "s2_32x5": (32, 5, False, 2), "transposed_33x64": (33, 64, True, 2)})
def _pack_table(ops, c, a, b, transposed, stride):
    w = c.t((a, b, 3, 3, 3))
    jobs = ops.unit_pack_jobs(w, transposed, stride)
    bufs = [c.out((ops.packed_floats(co, ci),)) for co, ci, _ in jobs]
    table = ops.make_pack_table([(w, buf, co, ci, m) for (co, ci, m), buf in zip(jobs, bufs)], w.device)
    ops.run_pack_table(table, len(jobs))
    return bufs


@cases("conv3d_k3_wgrad", "gradients", {"w13_b2_ci5": ((2, 5, 2, 3, 13), 32), "w24_ci32_co64": ((2, 32, 2, 2, 24), 64), "d1h1_w22_ci33": ((1, 33, 1, 1, 22), 32),
                                        "tiles_h9_w70": ((1, 8, 3, 9, 70), 32)})
def _wgrad3(ops, c, shape, Co):
    return [ops.conv3d_k3_wgrad(c.t(shape), c.t((shape[0], Co) + tuple(shape[2:])))]


_S2W = {"w13_b2_ci5": ((2, 5, 3, 4, 13), 32), "w24_ci32_co64": ((2, 32, 2, 4, 24), 64), "d1h1_w22": ((1, 16, 1, 1, 22), 32)}


@cases("conv3d_k3s2_wgrad", "gradients", _S2W)
def _wgrad_s2(ops, c, shape, Co):
    B, Ci, D, H, W = shape
    return [ops.conv3d_k3s2_wgrad(c.t(shape), c.t((B, Co, (D - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1)))]


@cases("deconv3d_k3s2_wgrad", "gradients", {"w5_b2_ci9": ((2, 9, 2, 2, 5), 32), "w12_ci32_co64": ((2, 32, 1, 2, 12), 64), "d1h1_w11": ((1, 16, 1, 1, 11), 7)})
def _wgrad_deconv(ops, c, shape, Co):
    B, Ci, D, H, W = shape
    return [ops.deconv3d_k3s2_wgrad(c.t(shape), c.t((B, Co, 2 * D, 2 * H, 2 * W)))]


@cases("conv3d_k3_dgrad", "gradients", {"s1_w13_ci5": ((2, 32, 2, 3, 13), 5, 1, None), "s1_w24_ci64": ((2, 32, 2, 2, 24), 64, 1, None),
                                        "s2_w7_ci32_odd": ((2, 64, 2, 2, 7), 32, 2, (3, 4, 13)), "s2_w12_ci96": ((1, 32, 1, 2, 12), 96, 2, None)})
def _dgrad3(ops, c, dshape, Ci, stride, in_size):
    B, Co = dshape[:2]
    size = tuple(in_size) if in_size is not None else tuple(stride * e for e in dshape[2:])
    return [ops.conv3d_k3_dgrad(c.t(dshape), c.t((Co, Ci, 3, 3, 3)), stride, in_size, residual=c.t((B, Ci) + size))]


@cases("deconv3d_k3s2_dgrad", "gradients", {"w26_ci9": ((2, 32, 4, 6, 26), 9), "w24_ci64": ((2, 32, 2, 4, 24), 64), "w2": ((1, 64, 2, 2, 2), 32)})
def _dgrad_deconv(ops, c, dshape, Ci):
    B, Co, D, H, W = dshape
    return [ops.deconv3d_k3s2_dgrad(c.t(dshape), c.t((Ci, Co, 3, 3, 3)), residual=c.t((B, Ci, D // 2, H // 2, W // 2)))]


# ================================================================================================ spatial propagation
_SPN = {"w13_b2": ((2, 3, 5, 13), True, False), "w24_rev": ((2, 2, 4, 24), True, True), "vert_w22": ((1, 2, 6, 22), False, False),
        "vert_rev_h1": ((1, 3, 1, 9), False, True), "w1": ((2, 2, 5, 1), True, False), "h64_w80": ((1, 2, 64, 80), True, False), "vert_h64_w80": ((1, 2, 64, 80), False, True)}


def _spn_ops(c, shape):
    g = [c.put(c.uni(shape, -0.3, 0.3)) for _ in range(3)]
    return c.t(shape), g[0], g[1], g[2]


@cases("spn_gaterecurrent2d", "spn", _SPN)
def _spn(ops, c, shape, horizontal, reverse):
    return [ops.spn_gaterecurrent2d(*_spn_ops(c, shape), horizontal, reverse)]


@cases("spn_gaterecurrent2d_bwd", "spn", _SPN)
def _spn_bwd(ops, c, shape, horizontal, reverse):
    X, G1, G2, G3 = _spn_ops(c, shape)
    Hf = ops.spn_gaterecurrent2d(X, G1, G2, G3, horizontal, reverse)
    return list(ops.spn_gaterecurrent2d_bwd(X, G1, G2, G3, Hf, c.t(shape), horizontal, reverse))


# ================================================================================================ AnyNet
_PRE = {"2d_w13_b2_ci5": ((2, 5, 6, 13), 8, 1, False), "2d_w24_ci64_pool": ((2, 64, 4, 24), 32, 1, True), "2d_s2_h1_w22": ((1, 3, 1, 22), 4, 2, False),
        "3d_w13_ci5": ((2, 5, 3, 2, 13), 16, 1, False), "3d_d1_w24": ((1, 16, 1, 3, 24), 1, 1, False), "2d_tiles_h33_w70": ((1, 8, 33, 70), 16, 1, False),
        "3d_tiles_h17_w70": ((1, 4, 3, 17, 70), 8, 1, False)}


@cases("preact_conv", "anynet", _PRE)
def _preact(ops, c, shape, Co, stride, pool):
    B, Ci = shape[:2]
    nd = len(shape) - 2
    w = c.t((Co, Ci) + (3,) * nd, 1.0 / (Ci * 3 ** nd) ** 0.5)
    ps, pb = c.affine(Ci)
    qs, qb = c.affine(Co)
    x, x2 = c.t((B, Ci + 2) + tuple(shape[2:])), c.t((B, Ci + 2) + tuple(shape[2:]))
    y = ops.preact_conv(x, w, stride, pool, ps, pb, True, qs, qb, True, None, False, in_window=(2, Ci))
    res = c.t(tuple(y.shape))
    plain = ops.preact_conv(x, w, stride, pool, None, None, False, None, None, False, res, False, in_window=(2, Ci))
    out = c.out((2 * B, Co + 3) + tuple(y.shape[2:]))
    ops.preact_conv(x, w, stride, pool, ps, pb, True, qs, qb, False, None, False, in_window=(2, Ci), x2=x2, out=out, out_ch_offset=1)
    return [y, plain, Win(out, (slice(None), slice(1, 1 + Co)))]


@cases("preact_conv", "anynet", {"gate_w13_b2": ((2, 8, 5, 13), 6), "gate_w24": ((1, 16, 3, 24), 24)})
def _preact_gate(ops, c, shape, Co):
    Ci = shape[1]
    return list(ops.preact_conv(c.t(shape), c.t((Co, Ci, 3, 3), 1.0 / (Ci * 9) ** 0.5), gate=True))


@cases("anynet_stage_samples", "anynet", {"w13_b2": ((2, 1, 3, 7), (6, 13), 5), "w24": ((2, 1, 2, 12), (4, 24), 3), "from_1x1_w22": ((1, 1, 1, 1), (2, 22), 2)})
def _stage_samples(ops, c, shape, size, D):
    low = c.t(shape, 3.0)
    return list(ops.anynet_stage_samples(low, size, 2.0, c.put(torch.linspace(-2.0, 2.0, D)))) + [ops.anynet_stage_samples(low, size, 2.0)[0]]


@cases("add", "anynet", {"n78_b2": (2, 1, 3, 13), "n96": (2, 2, 24), "n1": (1,), "n4099": (4099,)})
def _add(ops, c, *shape):
    return [ops.add(c.t(shape), c.t(shape))]


@cases("anynet_final_maps", "anynet", {"w13_b2": (2, (6, 13), ((6, 13), (3, 7), (2, 4), (1, 2))), "w24": (2, (4, 24), ((4, 24), (2, 12), (1, 6), (1, 3))),
                                       "h1_w22": (1, (1, 22), ((1, 22), (1, 11), (1, 6), (1, 3)))})
def _final_maps(ops, c, B, size, lows):
    return ops.anynet_final_maps([c.t((B, 1) + hw, 2.0) for hw in lows], size)


# ================================================================================================ DeepPruner's sampler
_PM = {"w13_b2_c5": ((2, 5, 4, 13), 3, False, True), "w24_c32_vert": ((2, 32, 3, 24), 5, True, True), "h2_w2_consts": ((1, 8, 2, 2), 1, False, False),
       "c33_w7": ((1, 33, 6, 7), 12, True, True), "h17_w41": ((1, 8, 17, 41), 5, False, True), "h17_w41_vert": ((1, 8, 17, 41), 5, True, True)}


@cases("patch_match_step", "patchmatch", _PM)
def _patch_match(ops, c, shape, P, vertical, maps):
    B, C, H, W = shape
    L, R, noise = c.t(shape), c.t(shape), c.put(c.uni((B, P, H, W)))
    lo = c.put(c.uni((B, 1, H, W), -3.0, 2.0)) if maps else None
    hi = c.put(c.uni((B, 1, H, W), 0.5 * W, W + 3.0)) if maps else None
    s, n = ops.patch_match_step(L, R, noise, lo, hi, vertical=vertical, bounds=(0.0, float(W)))
    out = c.out((B, P + 2, H, W))
    res, none = ops.patch_match_step(L, R, noise, lo, hi, vertical=vertical, bounds=(0.0, float(W)), want_noise=False, out=out)
    assert res is out and none is None
    return [s, n, out]      # (with ``out`` the range's ends land in channels 0 and P + 1: the whole tensor is written)


@cases("deeppruner_uniform_samples", "patchmatch", {"w13_b2_n5": ((2, 1, 3, 13), 5, None), "w24_n9_post": ((2, 1, 2, 24), 9, 48.0), "h1_w22_n2": ((1, 1, 1, 22), 2, None)})
def _uniform_samples(ops, c, shape, N, max_disp):
    lo = c.put(c.uni(shape, 0.0, 10.0))
    hi = c.put(c.uni(shape, 12.0, 40.0))
    return [ops.deeppruner_uniform_samples(lo, hi, N, max_disp)]


# ================================================================================================ preprocessing and metrics
@cases("stereo_pad_normalize", "preprocess_epe", {"f32_pad_b2": ("f32", (2, 3, 5, 13), None, (7, 16), True), "u8_window": ("u8", (2, 6, 14, 4), (1, 2, 4, 9), (6, 12), True),
                                                  "f32_gt_no_norm": ("f32", (1, 1, 3, 22), None, (3, 24), False), "u8_same_size": ("u8", (1, 4, 8, 3), None, None, True),
                                                  "f32_rows_w98": ("f32", (1, 3, 30, 98), None, (32, 100), True)})
def _pad_normalize(ops, c, kind, shape, window, size, norm):
    src = c.put(c.uni(shape, 0.0, 255.0).to(torch.uint8) if kind == "u8" else c.uni(shape, 0.0, 255.0))
    C = min(shape[3], 3) if kind == "u8" else shape[1]
    mean, std = (ops.IMAGENET_MEAN[:C], ops.IMAGENET_STD[:C]) if norm else (None, None)
    y = ops.stereo_pad_normalize(src, size, mean, std, window=window)
    out = c.out(tuple(y.shape))
    assert ops.stereo_pad_normalize(src, size, mean, std, window=window, out=out) is out
    return [y, out]


_EPE = {"w13_b2": ((2, 1, 5, 13), (4, 11)), "w24_b3": ((3, 1, 4, 24), (4, 24)), "h1_w22": ((1, 1, 1, 22), (1, 21)), "rows_70": ((1, 1, 70, 8), (66, 7))}


@cases("epe_accumulate", "preprocess_epe", _EPE)
def _epe(ops, c, shape, original):
    gt = c.uni(shape, -10.0, 210.0)
    est = c.put(gt + c.rand(shape, 3.0))
    acc = c.put(c.uni((6,), 0.0, 5.0).double(), inplace=True)          # the accumulator: updated in place (ops.epe_accumulate)
    assert ops.epe_accumulate(est, c.put(gt), acc, original, 0, 192) is acc
    return [acc]


@cases("epe_accumulate_multi", "preprocess_epe", _EPE)
def _epe_multi(ops, c, shape, original):
    gt = c.uni(shape, -10.0, 210.0)
    ests = [c.put(gt + c.rand(shape, 1.0 + i)) for i in range(3)]
    acc = c.put(c.uni((3, 6), 0.0, 5.0).double(), inplace=True)
    ops.epe_accumulate_multi(ests, c.put(gt), acc, original, 0, 192)
    one = c.put(torch.zeros((1, 6), dtype=torch.float64), inplace=True)
    ops.epe_accumulate_multi(ests[:1], c.put(gt), one, original, 0, 192)
    return [acc, one]


# ================================================================================================ the harness
def launching_wrappers():
    """Every public function of ``ops`` whose source launches a library kernel: through ``_lib.launch`` (directly, or by naming the
    entry point to the 3-D unit convolutions' shared launch body, ops._unit_conv3d) or through the shim."""
    ops = _ops()
    names = []
    for name, fn in vars(ops).items():
        if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != ops.__name__:
            continue
        src = inspect.getsource(fn)
        if 'launch("dmb_' in src or "_unit_conv3d(lib.dmb_" in src or re.search(r"\bsh\.\w+\(", src):
            names.append(name)
    return sorted(names)


def test_every_launching_wrapper_has_cases():
    """No exemptions: a new wrapper that launches a kernel needs calls in CASES before this module passes."""
    names = launching_wrappers()
    assert len(names) >= 69 and names[0] == "add" and names[-1] == "zero_columns_"
    missing = [n for n in names if n not in CASES]
    assert not missing, "launching wrappers without memory-contract cases: %s" % missing
    thin = [n for n in names if len(CASES[n]) < 2]
    assert not thin, "fewer than two calls for: %s" % thin
    unknown = [n for n in CASES if not hasattr(_ops(), n)]
    assert not unknown, unknown


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _flatten(res):
    return [] if res is None else list(res)


def _tensor(item):
    return item.tensor if isinstance(item, (Win, AtomicOrder)) else item


def _execute(case, dev, frame=None, misalign=0, shim=False):
    ops = _ops()
    c = Ctx(dev, case.seed, frame, misalign)
    try:
        if frame is None:
            res = case.body(ops, c, *case.args)
        else:
            with framed_library(frame, shim=shim):
                res = case.body(ops, c, *case.args)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e):     # a device fault: nothing more may run on this GPU in this session
            pytest.exit("device fault in %s: %s" % (case.id, str(e)[:300]), returncode=3)
        raise
    return c, _flatten(res)


def _snapshot(c, res):
    return ([None if r is None else _tensor(r).detach().cpu().clone() for r in res], [d.detach().cpu().clone() for _, d, _ in c.operands])


def _check_framed(case, dev, kind, misalign, plain, shim=False):
    what = "%s [%s pass%s%s]" % (case.id, kind, ", misaligned operands" if misalign else "", ", shim on" if shim else "")
    frame = Frame(kind, misalign=misalign)
    c, res = _execute(case, dev, frame, misalign, shim)
    p_res, p_ops = plain
    frame.check()                                                                                    # (a)
    if not shim:     # the frame was in effect: the wrapper's own allocations came from it (or it is known to make none)
        own = len(frame.buffers) - len(c.operands) - c.outs
        assert (own > 0) == (case.wrapper not in ALLOCATES_NOTHING), "%s: %d library allocations went through the frame" % (what, own)
    assert len(c.operands) == len(p_ops) and len(res) == len(p_res), what
    for i, ((cpu, d, inplace), p) in enumerate(zip(c.operands, p_ops)):                                # (b)
        assert _same_bits(d.cpu(), p if inplace else cpu), "%s: operand %d %s %s" % (
            what, i, tuple(cpu.shape), "differs from the plain run's updated value" if inplace else "was modified")
    for i, (r, p) in enumerate(zip(res, p_res)):
        if r is None or p is None:
            assert r is None and p is None, what
            continue
        t = _tensor(r)
        assert t.is_cuda, what
        if isinstance(r, Win):                                                                       # (e)
            inside = t[r.index]
            assert frame.unwritten(inside) == 0, "%s: result %d, %d window words unwritten" % (what, i, frame.unwritten(inside))
            assert frame.unwritten(t) == t.numel() - inside.numel(), "%s: result %d %s, %d words outside the window were written" % (
                what, i, tuple(t.shape), t.numel() - inside.numel() - frame.unwritten(t))
            assert _same_bits(inside, p[r.index]), "%s: result %d (window) differs from the plain run" % (what, i)
            continue
        left = frame.unwritten(t)                                                                    # (c)
        assert left == 0, "%s: result %d %s %s keeps %d unwritten words" % (what, i, tuple(t.shape), t.dtype, left)
        if isinstance(r, AtomicOrder):                                                               # (d), the one stated exception
            e_hip, e32 = (t.cpu().double() - r.truth).abs().max().item(), (r.ref32.double() - r.truth).abs().max().item()
            bound = 4 * e32 + 2e-6 * r.truth.abs().max().item()
            assert e_hip <= bound, "%s: result %d, |hip - fp64| = %g > %g" % (what, i, e_hip, bound)
            continue
        if not _same_bits(t, p):                                                                     # (d)
            a, b = t.detach().cpu().double().view(-1), p.double().view(-1)
            bad = (_bits(t).view(-1, t.element_size()) != _bits(p).view(-1, t.element_size())).any(1).nonzero().flatten()
            raise AssertionError("%s: result %d %s differs from the plain run in %d of %d elements, first at flat index %d: %r vs %r" % (
                what, i, tuple(t.shape), bad.numel(), a.numel(), int(bad[0]), a[int(bad[0])].item(), b[int(bad[0])].item()))
    for z in c.zeros:                                                                                # (g)
        assert int(z.ne(0).sum()) == 0, "%s: the work-queue workspace does not hold zeros after the call" % what


def _run_case(case, dev):
    from densematchingbenchmark_amd._lib import DmbLibraryError
    c, res = _execute(case, dev)
    plain = _snapshot(c, res)
    for z in c.zeros:
        assert int(z.ne(0).sum()) == 0
    for kind in ("nan", "huge"):
        _check_framed(case, dev, kind, 0, plain)
        if case.shim:                                                                                # (f)
            _check_framed(case, dev, kind, 0, plain, shim=True)
    if case.misalign == "ok":
        c, res = _execute(case, dev, misalign=4)
        plain = _snapshot(c, res)
        for kind in ("nan", "huge"):
            _check_framed(case, dev, kind, 4, plain)
    elif case.misalign == "refuse":
        with pytest.raises(DmbLibraryError):
            _execute(case, dev, misalign=4)
        with pytest.raises(DmbLibraryError):
            _execute(case, dev, Frame("nan", misalign=4), 4)
    else:
        assert case.misalign == "declines"       # conv3d_k3_bnstats: returns None for a misaligned input and launches nothing
        c, res = _execute(case, dev, misalign=4)
        assert res == []


def _family(name):
    return [pytest.param(k, id=k.id) for ks in CASES.values() for k in ks if k.family == name]


FAMILIES = sorted({k.family for ks in CASES.values() for k in ks})


def _make_test(family):
    @pytest.mark.parametrize("case", _family(family))
    def test(dev, case):
        _run_case(case, dev)
    test.__name__ = "test_%s" % family
    test.__doc__ = "The memory contract (module docstring) of the %s wrappers." % family
    return test


for _f in FAMILIES:
    globals()["test_%s" % _f] = _make_test(_f)
del _f
