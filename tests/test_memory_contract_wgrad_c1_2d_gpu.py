"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; every output word
written; results bit-identical to the plain run) for the 2-D one-output-channel weight gradient: plan form 7 of
dmb_conv_wgrad_plan (csrc/wgrad.hip), the way tests/test_memory_contract_wgrad_k5_gpu.py reuses that module.

Cases: two shapes of tests/test_wgrad_c1_2d_gpu.py -- "partial_tiles" (B = 2, so the last item's end is the operand's end; the last
tile partial on both axes: the halo reaches past every edge of the image, and past the operand's end; the most LDS) and "odd_width"
(rows of 13 floats, so every row starts at another alignment) -- plain, inside ``Frame("nan")`` and inside ``Frame("huge")``, with
both operands on a 16-byte boundary and 4, 8 and 12 bytes off it.  The form has no alignment rule, so every framed run must give
the bits of the one plain, aligned run.  The workspace is allocated inside the wrapper, so the frame guards AND poisons it: a
reduction that read a slot the plan does not use would not be bit-identical to the plain run.

test_workspace_of_exactly_the_planned_size hands the entry point a caller's workspace of slots x Ci x 9 floats, what the plan says
the launch uses and less than dmb_conv2d_wgrad_workspace_floats: every word of it is written, none next to it."""
import pytest
import torch

from tests._framed import Frame, framed_library
from tests.test_memory_contract_gpu import Case, Ctx, _check_framed, _execute, _same_bits, _snapshot
from tests.test_wgrad_c1_2d_gpu import CASES as C1_CASES, D2

pytestmark = pytest.mark.gpu
NAMES = ["partial_tiles", "odd_width"]


def _wgrad_c1(ops, c, name):
    xs, _ = C1_CASES[name]
    x, dc = c.t(xs), c.t((xs[0], 1) + xs[2:])
    assert ops.conv_wgrad_plan(D2, x, dc, 3, 1)[0] == 0x700
    return [ops.conv2d_wgrad(x, dc, 3, 1)]


CASES = [Case("conv2d_wgrad", "wgrad_c1_2d", name, _wgrad_c1, (name,), "ok", False) for name in NAMES]


@pytest.mark.parametrize("case", [pytest.param(k, id=k.id) for k in CASES])
def test_memory_contract(dev, case):
    c, res = _execute(case, dev)
    plain = _snapshot(c, res)
    c4, res4 = _execute(case, dev, misalign=4)        # plain memory, both operands 4 bytes off a 16-byte boundary
    assert _same_bits(res4[0].cpu(), plain[0][0]), "the alignment must not change the sums"
    for misalign in (0, 4, 8, 12):
        for kind in ("nan", "huge"):
            _check_framed(case, dev, kind, misalign, plain)


@pytest.mark.parametrize("name", NAMES)
def test_workspace_of_exactly_the_planned_size(dev, name):
    from densematchingbenchmark_amd import _lib, ops
    xs, _ = C1_CASES[name]
    B, Ci, H, W = xs
    ds = (B, 1, H, W)
    plan, (_, _, _, _, slots, blocks) = ops.conv_wgrad_plan(D2, xs, ds, 3, 1)
    used = slots * Ci * 9
    assert plan == 0x700 and blocks == 1 and used < _lib.load().dmb_conv2d_wgrad_workspace_floats(1, Ci)

    def body(c):
        x, dc = c.t(xs), c.t(ds)
        dw, ws = c.out((1, Ci, 3, 3)), c.out((used,))
        ops.launch("dmb_conv2d_wgrad_f32", x, dc, dw, ws, B, Ci, 1, H, W, 3, 1)
        torch.cuda.synchronize()
        return dw, ws
    plain_dw, plain_ws = body(Ctx(dev, 78))
    c = Ctx(dev, 78)
    x, dc = c.t(xs), c.t(ds)
    assert _same_bits(plain_dw, ops.conv2d_wgrad(x, dc, 3, 1))         # the wrapper's own, larger workspace: the same bits
    for kind in ("nan", "huge"):
        frame = Frame(kind)
        with framed_library(frame):
            dw, ws = body(Ctx(dev, 78, frame))
        frame.check()
        assert frame.unwritten(dw) == 0 and frame.unwritten(ws) == 0, "%s: unwritten words in the result or in the planned workspace" % kind
        assert _same_bits(dw, plain_dw) and _same_bits(ws, plain_ws)
