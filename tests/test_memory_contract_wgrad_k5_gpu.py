"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; every output word
written; results bit-identical to the plain run) for the 5x5 small-channel weight gradient: plan form 6 of dmb_conv_wgrad_plan
(csrc/wgrad.hip), the way tests/test_memory_contract_wgrad_hw_gpu.py reuses that module.

Cases: two shapes of tests/test_wgrad_k5_gpu.py -- "partial_tiles" (B = 2, so the last item's end is the operand's end; the last
tile partial on both axes: the halo reaches past every edge of the image, and past the operand's end) and "c14" (the most LDS; one
row group) -- plain, inside ``Frame("nan")`` and inside ``Frame("huge")``, and again with both operands 4 bytes off a 16-byte
boundary.  The workspace is allocated inside the wrapper, so the frame guards AND poisons it: a reduction that read a slot the plan
does not use would not be bit-identical to the plain run.

test_workspace_of_exactly_the_planned_size hands the entry point a caller's workspace of slots x Co x Ci x 25 floats, what the plan
says the launch uses and less than dmb_conv2d_wgrad_workspace_floats: every word of it is written, none next to it."""
import pytest
import torch

from tests._framed import Frame, framed_library
from tests.test_memory_contract_gpu import Case, Ctx, _check_framed, _execute, _same_bits, _snapshot
from tests.test_wgrad_k5_gpu import CASES as K5_CASES, D2

pytestmark = pytest.mark.gpu
NAMES = ["partial_tiles", "c14"]


def _wgrad_k5(ops, c, name):
    xs, Co, _ = K5_CASES[name]
    x, dc = c.t(xs), c.t((xs[0], Co) + xs[2:])
    assert ops.conv_wgrad_plan(D2, x, dc, 5, 1)[0] == 0x600
    return [ops.conv2d_wgrad(x, dc, 5, 1)]


CASES = [Case("conv2d_wgrad", "wgrad_k5", name, _wgrad_k5, (name,), "ok", False) for name in NAMES]


@pytest.mark.parametrize("case", [pytest.param(k, id=k.id) for k in CASES])
def test_memory_contract(dev, case):
    c, res = _execute(case, dev)
    plain = _snapshot(c, res)
    for kind in ("nan", "huge"):
        _check_framed(case, dev, kind, 0, plain)
    c, res = _execute(case, dev, misalign=4)          # both operands 4 bytes off a 16-byte boundary
    plain = _snapshot(c, res)
    for kind in ("nan", "huge"):
        _check_framed(case, dev, kind, 4, plain)


@pytest.mark.parametrize("name", NAMES)
def test_workspace_of_exactly_the_planned_size(dev, name):
    from densematchingbenchmark_amd import _lib, ops
    xs, Co, _ = K5_CASES[name]
    B, Ci, H, W = xs
    ds = (B, Co, H, W)
    plan, (_, _, _, _, slots, blocks) = ops.conv_wgrad_plan(D2, xs, ds, 5, 1)
    used = slots * Co * Ci * 25
    assert plan == 0x600 and blocks == 1 and used < _lib.load().dmb_conv2d_wgrad_workspace_floats(Co, Ci)

    def body(c):
        x, dc = c.t(xs), c.t(ds)
        dw, ws = c.out((Co, Ci, 5, 5)), c.out((used,))
        ops.launch("dmb_conv2d_wgrad_f32", x, dc, dw, ws, B, Ci, Co, H, W, 5, 1)
        torch.cuda.synchronize()
        return dw, ws
    plain_dw, plain_ws = body(Ctx(dev, 77))
    c = Ctx(dev, 77)
    x, dc = c.t(xs), c.t(ds)
    assert _same_bits(plain_dw, ops.conv2d_wgrad(x, dc, 5, 1))         # the wrapper's own, larger workspace: the same bits
    for kind in ("nan", "huge"):
        frame = Frame(kind)
        with framed_library(frame):
            dw, ws = body(Ctx(dev, 77, frame))
        frame.check()
        assert frame.unwritten(dw) == 0 and frame.unwritten(ws) == 0, "%s: unwritten words in the result or in the planned workspace" % kind
        assert _same_bits(dw, plain_dw) and _same_bits(ws, plain_ws)
