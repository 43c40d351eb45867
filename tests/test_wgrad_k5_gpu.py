"""The weight gradient of the stride-1 5x5 convolutions on 1 .. 16 channels (plan form 6 of dmb_conv_wgrad_plan, csrc/wgrad.hip)
alone, against torch's CPU autograd in FP64 and again in FP32:

    dw[co, ci, ky, kx] = sum_{b, y, x} dc[b, co, y, x] * x[b, ci, y + ky - 2, x + kx - 2]

through ``ops.conv2d_wgrad(x, dc, 5, 1)``.  The rule is that of tests/test_unit_grads_gpu.py: |hip - fp64| <= 4 |fp32 - fp64| +
2e-6 x range, and a second call is bit-identical (no atomics, fixed summation order).

CASES: the smallest shapes at which the kernel can go wrong.  Tiles are 8 rows x 32 columns; a thread owns one (co, ci) pair, and
where Co x Ci <= 128 the rows of a tile are dealt out to 256 / (Co x Ci) thread groups (at most 8).  Each case asserts its plan
through the query: (column tiles, row tiles, slots) on 256 compute units (512 slots)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests._large import binding
from tests.test_backward_gpu import _close
from tests.test_wgrad_hw_gpu import _off_by_4

pytestmark = pytest.mark.gpu
D2 = 4      # DMB_WGRAD_2D

# name: ((B, Ci, H, W), Co, (column tiles, row tiles, slots) at 256 compute units)
CASES = {
    "one_pixel": ((1, 1, 1, 1), 1, (1, 1, 1)),             # all taps but the centre see padding; 8 row groups, one row
    "below_halo": ((2, 3, 2, 3), 16, (1, 1, 2)),           # the image is smaller than the halo; 5 row groups
    "partial_tiles": ((2, 5, 19, 70), 3, (3, 3, 18)),      # 3 x 3 tiles, the last one partial on both axes; 8 row groups of 15 pairs
    "c14": ((2, 14, 16, 40), 14, (2, 2, 8)),               # DeepPruner's 14 -> 14: 196 threads, one row group
    "c16": ((1, 16, 24, 72), 16, (3, 3, 9)),               # every thread owns a pair
    "c9": ((2, 9, 9, 33), 9, (2, 2, 8)),                   # 9 -> 9: three row groups (rows 3 + 3 + 2), odd sizes
    "many_tiles": ((1, 1, 264, 520), 1, (17, 33, 512)),    # 561 tiles on 512 slots: items accumulate within a slot
}


def _autograd(x, dc, dtype):
    x, dc = x.to(dtype), dc.to(dtype)
    w = torch.zeros((dc.shape[1], x.shape[1], 5, 5), dtype=dtype, requires_grad=True)
    F.conv2d(x, w, None, stride=1, padding=2).backward(dc)
    return w.grad


@functools.lru_cache(maxsize=None)
def _data(name):
    """Operands (CPU, FP32) and the FP64 / FP32 autograd gradients of a case: computed once, never modified."""
    (B, Ci, H, W), Co, _ = CASES[name]
    g = torch.Generator().manual_seed(9600 + list(CASES).index(name))
    x, dc = torch.randn((B, Ci, H, W), generator=g), torch.randn((B, Co, H, W), generator=g)
    return x, dc, _autograd(x, dc, torch.float64), _autograd(x, dc, torch.float32)


@pytest.mark.parametrize("name", list(CASES))
def test_k5_weight_gradient_against_fp64_autograd(dev, name):
    from densematchingbenchmark_amd import ops
    (B, Ci, H, W), Co, tiles = CASES[name]
    x, dc, ref64, ref32 = _data(name)
    xd, dd = x.to(dev), dc.to(dev)
    plan, detail = ops.conv_wgrad_plan(D2, xd, dd, 5, 1)
    assert (plan, (detail[0], detail[3], detail[4])) == (0x600, tiles), "%s: this device plans 0x%03x %s" % (name, plan, detail)
    if name == "many_tiles":
        assert B * detail[0] * detail[3] > detail[4], "more items than slots"
    got = ops.conv2d_wgrad(xd, dd, 5, 1)
    assert got.shape == ref64.shape == (Co, Ci, 5, 5)
    _close(got.cpu(), ref64, ref32, "%s (plan 0x%03x)" % (name, plan))
    assert torch.equal(got, ops.conv2d_wgrad(xd, dd, 5, 1)), "%s: the weight gradient must be bit-reproducible (no atomics)" % name


def test_operands_4_bytes_off_a_16_byte_boundary(dev):
    """Neither operand 16-byte aligned, rows of 33 floats: the same form, the same bits as the aligned call"""
    from densematchingbenchmark_amd import ops
    for name in ("c9", "c14"):
        x, dc, ref64, ref32 = _data(name)
        xd, dd = _off_by_4(x, dev), _off_by_4(dc, dev)
        assert ops.conv_wgrad_plan(D2, xd, dd, 5, 1)[0] == 0x600
        got = ops.conv2d_wgrad(xd, dd, 5, 1)
        _close(got.cpu(), ref64, ref32, "%s, misaligned" % name)
        assert torch.equal(got, ops.conv2d_wgrad(xd, dd, 5, 1))
        assert torch.equal(got, ops.conv2d_wgrad(x.to(dev), dc.to(dev), 5, 1)), "the alignment must not change the sums"


@pytest.mark.parametrize("which", ["ctypes", "shim"])
def test_each_binding(dev, which):
    from densematchingbenchmark_amd import _lib, ops
    if which == "shim" and _lib.shim() is None:
        pytest.skip("the torch shim is not built: %s" % _lib.shim_state())
    x, dc, ref64, ref32 = _data("partial_tiles")
    with binding(which):
        got = ops.conv2d_wgrad(x.to(dev), dc.to(dev), 5, 1)
    _close(got.cpu(), ref64, ref32, "partial_tiles through %s" % which)
    assert torch.equal(got, ops.conv2d_wgrad(x.to(dev), dc.to(dev), 5, 1))


def test_other_kernel_5_shapes_are_still_refused(dev):
    from densematchingbenchmark_amd import _lib, ops
    x, dc = torch.zeros((1, 17, 8, 32), device=dev), torch.zeros((1, 16, 8, 32), device=dev)
    with pytest.raises(_lib.DmbLibraryError, match="kernel 1, or kernel 3"):
        ops.conv2d_wgrad(x, dc, 5, 1)
    with pytest.raises(_lib.DmbLibraryError, match="kernel 1, or kernel 3"):
        ops.conv2d_wgrad(x[:, :16].contiguous(), dc, 5, 2)
