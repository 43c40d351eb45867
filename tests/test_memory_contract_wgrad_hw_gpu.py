"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; every output word
written; results bit-identical to the plain run) for the weight gradient that strides only height and width: plan form 5 of
dmb_conv_wgrad_plan (csrc/wgrad.hip), the way tests/test_memory_contract_wgrad_forms_gpu.py reuses that module.

Cases: both instantiations (16-byte and dword staging) at shapes of tests/test_wgrad_hw_gpu.py -- B = 2 where the case has it, so
the last item's end is the operand's end; partial tiles on both axes; channel counts off the multiples of 32; odd big extents; the
minimum depth (the ring's z padding at both ends of a two-plane volume); segments of several planes with a shorter last one -- in
both roles, plain, inside ``Frame("nan")`` and inside ``Frame("huge")``, and again with both operands 4 bytes off a 16-byte boundary
(the dword instantiation on rows that would otherwise take 16-byte copies).  The workspace is allocated inside the wrappers, so the
frame guards AND poisons it: a reduction that read a slot the plan does not use would not be bit-identical to the plain run.

test_workspace_of_exactly_the_planned_size hands the entry point a caller's workspace of slots x blocks x 27 x 1024 floats, what the
plan says the launch uses and less than dmb_conv3d_wgrad_workspace_floats: every word of it is written, none next to it."""
import pytest
import torch

from tests._framed import Frame, framed_library
from tests.test_memory_contract_gpu import Case, Ctx, _check_framed, _execute, _same_bits, _snapshot
from tests.test_wgrad_hw_gpu import CASES as HW_CASES, S2

pytestmark = pytest.mark.gpu


def _wgrad_hw(ops, c, name, role):
    ss, sb, code, _ = HW_CASES[name]
    small, big = c.t(ss), c.t((ss[0],) + sb)
    want = 0x501 if c.misalign else code
    assert ops.conv_wgrad_plan(S2, small, big)[0] == want, "this device plans another instantiation than the case was recorded for"
    return [ops.conv3d_k3s2_wgrad(big, small) if role == "conv" else ops.deconv3d_k3s2_wgrad(small, big)]


_ROLES = [("min_depth", "conv"), ("min_depth", "transposed"), ("odd_big", "conv"), ("depth_14", "conv"), ("depth_14", "transposed"),
          ("deepest", "transposed"), ("one_voxel", "conv"), ("ring", "conv")]
CASES = [Case("conv3d_k3s2_wgrad" if role == "conv" else "deconv3d_k3s2_wgrad", "wgrad_hw", "%s_%s" % (name, role), _wgrad_hw, (name, role),
              "ok", False) for name, role in _ROLES]


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


@pytest.mark.parametrize("name", ["deepest", "odd_big"])
def test_workspace_of_exactly_the_planned_size(dev, name):
    from densematchingbenchmark_amd import _lib, ops
    ss, sb, code, _ = HW_CASES[name]
    plan, (_, _, _, _, slots, blocks) = ops.conv_wgrad_plan(S2, ss, (ss[0],) + sb)
    used = slots * blocks * 27 * 1024
    assert plan == code and used < _lib.load().dmb_conv3d_wgrad_workspace_floats(ss[1], sb[0])

    def body(c):
        small, big = c.t(ss), c.t((ss[0],) + sb)
        dw, ws = c.out((ss[1], sb[0], 3, 3, 3)), c.out((used,))
        ops.launch("dmb_conv3d_k3s2_wgrad_f32", small, big, dw, ws, ss[0], ss[1], sb[0], *ss[2:], *sb[1:])
        torch.cuda.synchronize()
        return dw, ws
    plain_dw, plain_ws = body(Ctx(dev, 77))
    small, big = _second(dev, ss, sb)
    assert _same_bits(plain_dw, ops.conv3d_k3s2_wgrad(big, small))         # the wrapper's own, larger workspace: the same bits
    for kind in ("nan", "huge"):
        frame = Frame(kind)
        with framed_library(frame):
            dw, ws = body(Ctx(dev, 77, frame))
        frame.check()
        assert frame.unwritten(dw) == 0 and frame.unwritten(ws) == 0, "%s: unwritten words in the result or in the planned workspace" % kind
        assert _same_bits(dw, plain_dw) and _same_bits(ws, plain_ws)


def _second(dev, ss, sb):
    """The operands ``body`` draws from seed 77, on plain memory: (small, big)"""
    c = Ctx(dev, 77)
    return c.t(ss), c.t((ss[0],) + sb)
