"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; every output word
written; results bit-identical to the plain run) for EVERY instantiation the weight-gradient wrappers can plan: the 13 codes of
dmb_conv_wgrad_plan (csrc/wgrad.hip).

That module's weight-gradient rows use widths 5 .. 24 (70 for one output channel): they take the 24-column stride-1 tile and the
2 x 12 stride-2 tile only, mostly in one segment.  The 32-column stride-1 kernel and both 4 x 8 stride-2 kernels never ran between
guard pages: their partial-tile masks, their out-of-range copies and a short last segment are what this module adds.  Here: one
launch per plan code from GPU_CASES of tests/test_wgrad_plan_host.py -- B = 2, so that the last item's end is the operand's end, a
partial last tile on every tiled axis, a channel count off the multiples of 32 (the last channel block ends inside the operand's
last item), two or more segments with a shorter last one --; plain, inside ``Frame("nan")`` and inside ``Frame("huge")``, rules
(a) - (e) of that module through its ``_check_framed``.  The workspace is allocated inside the wrappers, so the frame guards it
too.  Each body first asserts that the launch it is about to make has the recorded plan on this device."""
import pytest

from tests.test_memory_contract_gpu import Case, Ctx, _check_framed, _execute, _snapshot  # noqa: F401  (Ctx: the type a body receives)
from tests.test_wgrad_plan_host import D2, GPU_CASES, S2, gpu_case_shapes

pytestmark = pytest.mark.gpu


def _wgrad_form(ops, c, case):
    _, kind, _, _, _, k, dl, code, _ = case
    sa, sb = gpu_case_shapes(case)
    a, b = c.t(sa), c.t(sb)
    assert ops.conv_wgrad_plan(kind, a, b, k, dl)[0] == code, "this device plans another instantiation than the case was recorded for"
    if kind == D2:
        return [ops.conv2d_wgrad(a, b, k, dl)]
    return [ops.conv3d_k3s2_wgrad(b, a) if kind == S2 else ops.conv3d_k3_wgrad(a, b)]


_WRAPPER = {D2: "conv2d_wgrad", S2: "conv3d_k3s2_wgrad"}
CASES = [Case(_WRAPPER.get(case[1], "conv3d_k3_wgrad"), "wgrad_forms", "%s_plan_%03x" % (case[0], case[7]), _wgrad_form, (case,), "ok", False)
         for case in GPU_CASES]


@pytest.mark.parametrize("case", [pytest.param(k, id=k.id) for k in CASES])
def test_memory_contract(dev, case):
    c, res = _execute(case, dev)
    plain = _snapshot(c, res)
    for kind in ("nan", "huge"):
        _check_framed(case, dev, kind, 0, plain)
