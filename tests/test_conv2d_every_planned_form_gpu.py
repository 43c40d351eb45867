"""Every instantiation dmb_conv2d_f32 can plan -- the 33 tiles of csrc/conv2d.hip and the four split-K variants of
csrc/conv3d_sk.hip -- run at its smallest launch and compared pixel by pixel with an FP64 convolution.

Which instantiation a launch takes follows the layer (kernel, stride, dilation, channel width), the 16-byte alignment of its rows and,
for the tile height of 64-channel 3x3 layers and for split-K, the launch's SIZE: the small shapes of tests/test_kernels_gpu.py take
two rows per wave or split-K, so the four-row 64-channel tile ran in whole-model tests only.  tests/test_conv2d_plan_host.py:
GPU_CASES holds one shape per code: two or more tiles and a PARTIAL last tile along x and y of that code's tile (the zero fill of the
staging and the masks of the epilogue are what a tile can get wrong without a full image noticing), a partial 16 x 2 unit along both
axes for split-K.

Per case: the plan of the launch about to be made (real alignments, this device's compute units) is the recorded one -- a device
with another CU count fails here by name instead of testing other kernels --; plain, and folded affine + skip + ReLU, each into a
fresh tensor and into a channel window of a wider, NaN-filled ``out=`` whose other channels must still be NaN afterwards, against
F.conv2d in FP64 on the CPU: unit-variance inputs, weights scaled by 1 / sqrt(Ci k k), so outputs are O(1) and the bound is the
project's 2e-5 for one such layer (tests/test_kernels_gpu.py).  A failure names the worst output's (b, c, y, x) and where it sits
inside its tile.

Under the single-chain flag every batch item run alone -- another tile height for the four-row case, asserted -- is bit-identical to
its slice of the batch; and every vector tile equals the scalar tile of the same layer on a misaligned copy of the input
(include/dmb_hip.h: ONE k-ordered fma chain per output whatever the tile)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv2d_plan_host import GPU_CASES, SPLIT_K, TILES, TX, scalar_of

pytestmark = pytest.mark.gpu
BOUND = 2e-5
_BY_NAME = {c[0]: c for c in GPU_CASES}
_IDS = [c[0] for c in GPU_CASES]
MODES = {"plain": (False, False, False), "skip_relu": (True, True, True)}   # affine, skip, relu
PAD_CH, OFF_CH = 5, 2     # the wider out= tensor: Co + 5 channels, written from channel 2


def _ops():
    from densematchingbenchmark_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _data(name):
    """The case's operands (CPU, FP32) and the FP64 convolution of them: computed once, shared by the tests below, never modified."""
    _, Ci, Co, k, s, dl, (B, H, W), _, _ = _BY_NAME[name]
    g = torch.Generator().manual_seed(3000 + _IDS.index(name))
    x = torch.randn((B, Ci, H, W), generator=g)
    w = torch.randn((Co, Ci, k, k), generator=g) / math.sqrt(Ci * k * k)
    sc, sh = 0.5 + torch.rand(Co, generator=g), torch.rand(Co, generator=g) - 0.5     # a folded BatchNorm
    conv = F.conv2d(x.double(), w.double(), None, stride=s, padding=dl * (k // 2), dilation=dl)
    res = torch.randn(conv.shape, generator=g)
    return x, w, sc, sh, res, conv


def _expected(name, mode):
    _, _, sc, sh, res, conv = _data(name)
    affine, skip, relu = MODES[mode]
    ref = conv * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1) if affine else conv
    if skip:
        ref = ref + res.double()
    return F.relu(ref) if relu else ref


def _where(code, idx):
    """'(b, c, y, x), tile-local ...' of an output index, for the failure message."""
    b, c, y, x = idx
    if code in SPLIT_K:
        return "(b, c, y, x) = %s, (x, y) = (%d, %d) inside its 16 x 2 unit" % (idx, x % 16, y % 2)
    ty = TILES[code & 0xff][5]
    return "(b, c, y, x) = %s, (x, y) = (%d, %d) inside its %d x %d tile" % (idx, x % TX, y % ty, TX, ty)


def _assert_close(got, ref, code, what):
    err = (got.double().cpu() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)     # an unwritten (NaN) output is the worst one
    worst = err.max().item()
    print("%s: max |hip - fp64| = %.3g" % (what, worst))
    if worst > BOUND:
        idx = tuple(int(v) for v in torch.unravel_index(err.argmax(), err.shape))
        raise AssertionError("%s (plan 0x%03x): |hip - fp64| = %g > %g at %s: got %r, expected %r; %d of %d outputs beyond the bound" % (
            what, code, worst, BOUND, _where(code, idx), got[idx].item(), ref[idx].item(), int((err > BOUND).sum()), err.numel()))


def _device_args(name, dev):
    x, w, sc, sh, res, conv = _data(name)
    ops = _ops()
    return x.to(dev), ops.pack_conv2d_weights(w.to(dev)), sc.to(dev), sh.to(dev), res.to(dev)


def _misaligned(t):
    """A copy 4 bytes off the allocator's alignment."""
    return torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape).copy_(t)


@pytest.mark.parametrize("name", _IDS)
def test_every_planned_form_against_fp64(dev, name):
    ops = _ops()
    _, Ci, Co, k, s, dl, shape, code, _ = _BY_NAME[name]
    xd, wp, scd, shd, resd = _device_args(name, dev)
    conv = _data(name)[5]
    B, _, Ho, Wo = conv.shape
    for mode, (affine, skip, relu) in MODES.items():
        ref = _expected(name, mode)
        a_sc, a_sh, a_res = (scd if affine else None, shd if affine else None, resd if skip else None)
        for into in ("fresh", "window"):
            out = None if into == "fresh" else torch.full((B, Co + PAD_CH, Ho, Wo), float("nan"), device=dev)
            off = 0 if out is None else OFF_CH
            # first: this launch, on this device, is the instantiation the case is there for
            plan = ops.conv2d_plan(xd, Co, k, s, dl, a_res, out=out, out_ch_offset=off)
            assert plan == code, "%s: this device plans 0x%03x for the launch, the case was recorded for 0x%03x at 256 compute units" % (name, plan, code)
            got = ops.conv2d(xd, wp, Co, k, s, dl, a_sc, a_sh, a_res, relu, out=out, out_ch_offset=off)
            if out is not None:
                assert got.data_ptr() == out.data_ptr()
                rest = torch.cat((out[:, :off], out[:, off + Co:]), dim=1)
                assert bool(torch.isnan(rest).all()), "%s %s: channels outside the window were written" % (name, mode)
                got = out[:, off:off + Co]
            _assert_close(got, ref, code, "%s %s %s" % (name, mode, into))


@pytest.mark.parametrize("name", _IDS)
@pytest.mark.usefixtures("single_chain")
def test_batch_item_alone_is_bit_identical(dev, name):
    ops = _ops()
    _, Ci, Co, k, s, dl, shape, code, alone = _BY_NAME[name]
    xd, wp, scd, shd, resd = _device_args(name, dev)
    plan = ops.conv2d_plan(xd, Co, k, s, dl, resd)
    if code in SPLIT_K:      # (the flag keeps the batch off split-K: some tile)
        assert plan >> 8 == ops.CONV2D_PLAN_TILES
    else:
        assert plan == code
    both = ops.conv2d(xd, wp, Co, k, s, dl, scd, shd, resd, True)
    for b in range(shape[0]):
        xb, rb = xd[b:b + 1].clone(), resd[b:b + 1].clone()      # (fresh allocations: 16-byte aligned like the batch)
        assert ops.conv2d_plan(xb, Co, k, s, dl, rb) == alone, "%s: item alone plans another code than recorded" % name
        one = ops.conv2d(xb, wp, Co, k, s, dl, scd, shd, rb, True)
        if not torch.equal(one[0], both[b]):
            diff = (one[0] != both[b])
            idx = (b,) + tuple(int(v) for v in torch.unravel_index(diff.int().argmax(), diff.shape))
            raise AssertionError("%s: batch item %d alone (plan 0x%03x) differs from its slice of the batch (plan 0x%03x) in %d outputs, first at %s" % (
                name, b, alone, plan, int(diff.sum()), _where(plan, idx)))


_VECTOR = [c[0] for c in GPU_CASES if c[7] not in SPLIT_K and TILES[c[7] & 0xff][4]]


@pytest.mark.parametrize("name", _VECTOR)
def test_vector_tile_equals_the_scalar_tile_on_a_misaligned_copy(dev, name):
    ops = _ops()
    _, Ci, Co, k, s, dl, shape, code, _ = _BY_NAME[name]
    xd, wp, scd, shd, resd = _device_args(name, dev)
    xm = _misaligned(xd)
    assert ops.conv2d_plan(xd, Co, k, s, dl, resd) == code
    assert ops.conv2d_plan(xm, Co, k, s, dl, resd) == scalar_of(code)
    vec = ops.conv2d(xd, wp, Co, k, s, dl, scd, shd, resd, True)
    scalar = ops.conv2d(xm, wp, Co, k, s, dl, scd, shd, resd, True)
    if not torch.equal(vec, scalar):
        diff = (vec != scalar)
        idx = tuple(int(v) for v in torch.unravel_index(diff.int().argmax(), diff.shape))
        raise AssertionError("%s: the vector tile (plan 0x%03x) differs from the scalar one (0x%03x) in %d outputs, first at %s" % (
            name, code, scalar_of(code), int(diff.sum()), _where(code, idx)))
