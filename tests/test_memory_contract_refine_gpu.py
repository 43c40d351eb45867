"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; no unwritten output
word; results bit-identical to the plain run; 4-byte aligned operands) for ``ops_deeppruner.refine_head_up2``
(csrc/refine_head.hip) and for one whole ``DeepPrunerRefinement`` cascade.  The cases are built here and run by that module's
``_run_case`` (both poison kinds, and the pass with operands 4 bytes off a 16-byte boundary); the passes 8 and 12 bytes off are
added below with the same helpers, as tests/test_memory_contract_deeppruner_gpu.py does.  That module's own table is not touched.

Head shapes: one pixel, one row, B = 2 with an odd channel count below one tile, and several 32 x 8 tiles with partial ones on both
edges.  The cascade is the two-stage one (the 8x config's widths, batch 2): its guide buffers, every layer's output and the packed
weights come from the frame; the up-sampled maps are the results, the disparity and the guide features the operands."""
import pytest
import torch

from densematchingbenchmark_amd import ops_deeppruner
from densematchingbenchmark_amd.modeling.stereo.disp_refinement import DeepPrunerRefinement
from tests import _deeppruner_features_ref as R
from tests.test_memory_contract_gpu import Case, Ctx, Frame, _check_framed, _execute, _run_case, _snapshot  # noqa: F401  (Ctx: the type a body receives)

pytestmark = pytest.mark.gpu


def _head(ops, c, shape):
    B, Ci, H, W = shape
    return [ops_deeppruner.refine_head_up2(c.t(shape), c.t((1, Ci, 3, 3), 1.0 / (Ci * 9) ** 0.5), c.t((B, 1, H, W)))]


def _cascade(ops, c, name):
    (planes, num, _, _), _ = R.REFINE_CASES[name]
    hip = DeepPrunerRefinement(list(planes), True, num)
    hip.load_state_dict(R.refinement(name).state_dict(), strict=True)
    hip = hip.to(c.dev).eval()
    disps, fms = R.refine_inputs(name)
    with torch.no_grad():
        out = hip([c.put(disps[0])], [c.put(t) for t in fms])
    return out[:-1]                                                          # (the last one is the operand itself)


_SHAPES = {
    "refine_head_up2": (_head, {"one_pixel": ((1, 1, 1, 1),), "h1_w22": ((1, 16, 1, 22),), "w13_b2_ci5": ((2, 5, 5, 13),),
                                "tiles_h17_w70": ((1, 16, 17, 70),)}),
    "DeepPrunerRefinement": (_cascade, {"two_stages_b2": ("r8x",)}),
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
