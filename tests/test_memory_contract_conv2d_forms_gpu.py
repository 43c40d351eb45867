"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; every output word
written; results bit-identical to the plain run) for EVERY instantiation ``ops.conv2d`` can plan: the 33 tiles of csrc/conv2d.hip
and the four split-K variants of csrc/conv3d_sk.hip.

That module's ``conv2d`` table runs tiny edge shapes, which take two rows per wave, split-K or a single tile: the partial-tile zero
fill and the epilogue masks of the other instantiations never ran between guard pages.  Here: one launch per plan code from GPU_CASES
of tests/test_conv2d_plan_host.py -- the smallest shape that reaches the code with a partial last tile along x and y of that tile,
B = 2 so that the last item's end is the operand's end -- with folded affine, skip operand and ReLU, into a fresh tensor and into a
channel window of the caller's wider ``out=``, reading a channel window of a wider input; plain, inside ``Frame("nan")`` and inside
``Frame("huge")``, rules (a) - (e) of that module through its ``_check_framed``.  Each body first asserts that the launch it is about
to make has the recorded plan on this device."""
import pytest

from tests.test_conv2d_plan_host import GPU_CASES
from tests.test_memory_contract_gpu import Case, Ctx, Win, _check_framed, _execute, _snapshot  # noqa: F401  (Ctx: the type a body receives)

pytestmark = pytest.mark.gpu


def _conv2d_form(ops, c, Ci, Co, k, stride, dil, shape, code):
    B, H, W = shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    wp = ops.pack_conv2d_weights(c.t((Co, Ci, k, k), 1.0 / (Ci * k * k) ** 0.5))
    sc, sh = c.affine(Co)
    x = c.t((B, Ci + 3, H, W))                                        # read through a channel window
    res = c.t((B, Co + 2, Ho, Wo))
    out = c.out((B, Co + 5, Ho, Wo))
    kw = dict(in_window=(3, Ci), res_ch_offset=2)
    assert ops.conv2d_plan(x, Co, k, stride, dil, res, **kw) == code, "this device plans another instantiation than the case was recorded for"
    y = ops.conv2d(x, wp, Co, k, stride, dil, sc, sh, res, True, **kw)
    assert ops.conv2d_plan(x, Co, k, stride, dil, res, out=out, out_ch_offset=4, **kw) == code
    ops.conv2d(x, wp, Co, k, stride, dil, sc, sh, res, True, out=out, out_ch_offset=4, **kw)
    return [y, Win(out, (slice(None), slice(4, 4 + Co)))]


CASES = [Case("conv2d", "conv2d_forms", "%s_plan_%03x" % (name, code), _conv2d_form, (Ci, Co, k, s, dl, shape, code), "ok", False)
         for name, Ci, Co, k, s, dl, shape, code, _ in GPU_CASES]


@pytest.mark.parametrize("case", [pytest.param(k, id=k.id) for k in CASES])
def test_memory_contract(dev, case):
    c, res = _execute(case, dev)
    plain = _snapshot(c, res)
    for kind in ("nan", "huge"):
        _check_framed(case, dev, kind, 0, plain)
