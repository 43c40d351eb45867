"""The weight gradient of a stride-1 3x3 convolution with ONE output channel on 1 .. 16 input channels (plan form 7 of
dmb_conv_wgrad_plan, csrc/wgrad.hip: the classifier of DeepPruner's refinement head) alone, against torch's CPU
``torch.nn.grad.conv2d_weight`` in FP64 and again in FP32:

    dw[0, ci, ky, kx] = sum_{b, y, x} dc[b, 0, y, x] * x[b, ci, y + ky - 1, x + kx - 1]

through ``ops.conv2d_wgrad(x, dc, 3, 1)``.  The rule is that of tests/test_wgrad_k5_gpu.py: |hip - fp64| <= 4 |fp32 - fp64| +
2e-6 x range, and a second call is bit-identical (no atomics, fixed summation order).

CASES: the head's own six shapes.  Tiles are 8 rows x 32 columns in 32 units of (row, 8 columns); a thread owns one input channel
and belongs to one of min(256 / Ci, 32) groups.  Each case asserts its plan through the query: on the parent commit these
descriptions plan 0x400 (form 4) or, at a width that is no multiple of 4, are padded by the wrapper first."""
import functools

import pytest
import torch

from tests._large import binding
from tests.test_backward_gpu import _close
from tests.test_wgrad_hw_gpu import _off_by_4

pytestmark = pytest.mark.gpu
D2 = 4      # DMB_WGRAD_2D

# name: ((B, Ci, H, W), (column tiles, row tiles))
CASES = {
    "one_pixel": ((1, 1, 1, 1), (1, 1)),              # all taps but the centre see padding; 32 groups of one thread
    "one_row": ((1, 16, 1, 22), (1, 1)),              # 16 groups; rows 1 .. 7 of the tile are skipped
    "odd_width": ((2, 5, 5, 13), (1, 1)),             # 32 groups of 5 threads, 160 of 256 threads own sums
    "partial_tiles": ((2, 16, 17, 70), (3, 3)),       # 3 x 3 tiles, the last one partial on both axes
    "narrow": ((1, 9, 40, 8), (1, 5)),                # 28 groups: units 28 .. 31 go to groups 0 .. 3 in a second round
    "odd_past_a_tile": ((1, 16, 33, 65), (3, 5)),     # one row and one column past a tile boundary
}


def _weight_grad(x, dc, dtype):
    x, dc = x.to(dtype), dc.to(dtype)
    return torch.nn.grad.conv2d_weight(x, (1, x.shape[1], 3, 3), dc, stride=1, padding=1)


@functools.lru_cache(maxsize=None)
def _data(name):
    """Operands (CPU, FP32) and the FP64 / FP32 gradients of a case: computed once, never modified."""
    (B, Ci, H, W), _ = CASES[name]
    g = torch.Generator().manual_seed(9700 + list(CASES).index(name))
    x, dc = torch.randn((B, Ci, H, W), generator=g), torch.randn((B, 1, H, W), generator=g)
    return x, dc, _weight_grad(x, dc, torch.float64), _weight_grad(x, dc, torch.float32)


@pytest.mark.parametrize("name", list(CASES))
def test_c1_weight_gradient_against_fp64(dev, name):
    from densematchingbenchmark_amd import ops
    (B, Ci, H, W), tiles = CASES[name]
    x, dc, ref64, ref32 = _data(name)
    xd, dd = x.to(dev), dc.to(dev)
    plan, detail = ops.conv_wgrad_plan(D2, xd, dd, 3, 1)
    assert (plan, (detail[0], detail[3])) == (0x700, tiles), "%s: this device plans 0x%03x %s" % (name, plan, detail)
    assert plan >> 8 == ops.WGRAD_PLAN_C1_2D and detail[4] == B * tiles[0] * tiles[1]     # fewer items than slots: one tile per slot
    got = ops.conv2d_wgrad(xd, dd, 3, 1)
    assert got.shape == ref64.shape == (1, Ci, 3, 3)
    _close(got.cpu(), ref64, ref32, "%s (plan 0x%03x)" % (name, plan))
    assert torch.equal(got, ops.conv2d_wgrad(xd, dd, 3, 1)), "%s: the weight gradient must be bit-reproducible (no atomics)" % name


def test_operands_4_bytes_off_a_16_byte_boundary(dev):
    """Neither operand 16-byte aligned, odd widths: the same form, the same bits as the aligned call"""
    from densematchingbenchmark_amd import ops
    for name in ("odd_width", "odd_past_a_tile"):
        x, dc, ref64, ref32 = _data(name)
        xd, dd = _off_by_4(x, dev), _off_by_4(dc, dev)
        assert ops.conv_wgrad_plan(D2, xd, dd, 3, 1)[0] == 0x700
        got = ops.conv2d_wgrad(xd, dd, 3, 1)
        _close(got.cpu(), ref64, ref32, "%s, misaligned" % name)
        assert torch.equal(got, ops.conv2d_wgrad(xd, dd, 3, 1))
        assert torch.equal(got, ops.conv2d_wgrad(x.to(dev), dc.to(dev), 3, 1)), "the alignment must not change the sums"


def test_both_bindings_give_equal_results(dev):
    from densematchingbenchmark_amd import _lib, ops
    assert _lib.shim() is not None, "the torch shim is not built: %s" % _lib.shim_state()
    for name in ("partial_tiles", "narrow"):
        x, dc, ref64, ref32 = _data(name)
        got = {}
        for which in ("ctypes", "shim"):
            with binding(which):
                got[which] = ops.conv2d_wgrad(x.to(dev), dc.to(dev), 3, 1)
            _close(got[which].cpu(), ref64, ref32, "%s through %s" % (name, which))
        assert torch.equal(got["ctypes"], got["shim"]), name


def test_more_items_than_slots(dev):
    """Items accumulate within a slot: 2 x 9 x 65 = 1170 tiles of a [2, 3, 68, 2070] map on 4 slots per compute unit"""
    from densematchingbenchmark_amd import ops
    g = torch.Generator().manual_seed(9790)
    x, dc = torch.randn((2, 3, 68, 2070), generator=g), torch.randn((2, 1, 68, 2070), generator=g)
    xd, dd = x.to(dev), dc.to(dev)
    plan, detail = ops.conv_wgrad_plan(D2, xd, dd, 3, 1)
    assert plan == 0x700 and 2 * detail[0] * detail[3] == 1170 > detail[4], detail
    got = ops.conv2d_wgrad(xd, dd, 3, 1)
    _close(got.cpu(), _weight_grad(x, dc, torch.float64), _weight_grad(x, dc, torch.float32), "more items than slots")
    assert torch.equal(got, ops.conv2d_wgrad(xd, dd, 3, 1))


def test_neighbouring_descriptions_keep_form_4(dev):
    from densematchingbenchmark_amd import _lib, ops
    x, dc = torch.zeros((1, 17, 8, 64), device=dev), torch.zeros((1, 1, 8, 64), device=dev)
    assert ops.conv_wgrad_plan(D2, x, dc, 3, 1)[0] == 0x400
    assert ops.conv_wgrad_plan(D2, x[:, :16].contiguous(), dc, 3, 2)[0] == 0x401
    assert ops.conv_wgrad_plan(D2, x[:, :16].contiguous(), dc, 1, 1)[0] == 0x404
    assert ops.conv2d_wgrad(x, dc, 3, 1).shape == (1, 17, 3, 3)
    with pytest.raises(_lib.DmbLibraryError, match="kernel 1, or kernel 3"):
        ops.conv2d_wgrad(x[:, :16].contiguous(), dc, 3, 3)
