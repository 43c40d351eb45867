"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; no unwritten output
word; results bit-identical to the plain run; 4-byte aligned operands) for the two launching wrappers of
``densematchingbenchmark_amd.ops_deeppruner`` (csrc/deeppruner_heads.hip).  The cases are built here and run by that module's
``_run_case`` (both poison kinds, and the pass with operands 4 bytes off a 16-byte boundary); the passes 8 and 12 bytes off are
added below with the same helpers.  That module's own table is not touched.

Volume shapes: W % 4 == 1 with B = 2, the builder's minimum of two rows and two planes, no feature maps (stage "pre"), and several
blocks along a row-major plane with a partial last one.  Convolution shapes: one pixel, one row, B = 2 with channel counts off
every tile of four, and several 32 x 8 tiles with partial ones on both edges."""
import pytest

from densematchingbenchmark_amd import ops_deeppruner
from tests.test_memory_contract_gpu import Case, Ctx, Frame, _check_framed, _execute, _run_case, _snapshot  # noqa: F401  (Ctx: the type a body receives)

pytestmark = pytest.mark.gpu


def _volume(ops, c, shape, D, P):
    B, C, H, W = shape
    s = c.put(c.uni((B, D, H, W), -2.0, 1.2 * W))
    feats = (c.t((B, P, H, W)), c.t((B, P, H, W))) if P else ()
    return [ops_deeppruner.deeppruner_volume(c.t(shape), c.t(shape), s, *feats)]


def _conv(ops, c, shape, Co, epilogue):
    B, Ci, H, W = shape
    w = c.t((Co, Ci, 5, 5), 1.0 / (Ci * 25) ** 0.5)
    sc, sh = c.affine(Co) if epilogue == "affine" else (None, c.put(c.uni((Co,), -0.5, 0.5)) if epilogue == "bias" else None)
    return [ops_deeppruner.conv2d_k5_small(c.t(shape), w, sc, sh, epilogue != "none")]


_SHAPES = {
    "deeppruner_volume": (_volume, {"w13_b2": ((2, 5, 3, 13), 4, 3), "w22_h2_d2": ((1, 3, 2, 22), 2, 1), "p0": ((2, 4, 3, 10), 3, 0),
                                    "blocks_w70": ((1, 4, 5, 70), 6, 2)}),
    "conv2d_k5_small": (_conv, {"one_pixel": ((1, 1, 1, 1), 1, "bias"), "h1_w22": ((1, 9, 1, 22), 9, "affine"),
                                "w13_b2_ci5": ((2, 5, 3, 13), 3, "none"), "tiles_h17_w70": ((1, 14, 17, 70), 14, "affine")}),
}

CASES = [Case(_wrapper, "deeppruner", _label, _body, _args, "ok", False)
         for _wrapper, (_body, _calls) in _SHAPES.items() for _label, _args in _calls.items()]


@pytest.mark.parametrize("case", [pytest.param(k, id=k.id) for k in CASES])
def test_memory_contract(dev, case):
    _run_case(case, dev)
    for misalign in (8, 12):        # the frame's operands 8 and 12 bytes off a 16-byte boundary, against a plain run 4 bytes off
        c, res = _execute(case, dev, misalign=misalign)
        plain = _snapshot(c, res)
        for kind in ("nan", "huge"):
            _check_framed(case, dev, kind, misalign, plain)
