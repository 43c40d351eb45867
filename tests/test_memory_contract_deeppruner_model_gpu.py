"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; no unwritten output
word; results bit-identical to the plain run; 4-byte aligned operands) for ``ops_deeppruner.deeppruner_final_maps``
(csrc/deeppruner_final_maps.hip) and for one whole forward of the ``DeepPruner`` model.  The cases are built here and run by that
module's ``_run_case`` (both poison kinds, and the pass with operands 4 bytes off a 16-byte boundary); the passes 8 and 12 bytes
off are added below with the same helpers, as tests/test_memory_contract_refine_gpu.py does.  That module's own table is not touched.

Tail shapes (B, H, W, K; the list at (H >> k, W >> k), the range maps at (H >> K, W >> K)): 4 x 4 down to 1 x 1 maps; B = 2 with
24 columns, less than one 64-column tile; odd quarter and eighth sizes; several tiles with a partial last one and B = 2.  The
forward is the 8x config's at the recorded shape (batch 2, two refinement stages): the images and PatchMatch's noise are the
operands, the K + 4 = 7 output maps the results; every intermediate and the packed weights come from the frame."""
import os

import pytest
import torch

from densematchingbenchmark_amd import ops_deeppruner
from densematchingbenchmark_amd.config import Config
from densematchingbenchmark_amd.modeling.stereo.models import DeepPruner
from tests import _deeppruner_model_ref as R
from tests.test_memory_contract_gpu import Case, Ctx, Frame, _check_framed, _execute, _run_case, _snapshot  # noqa: F401  (Ctx: the type a body receives)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tail(ops, c, B, H, W, K):
    disps = [c.put(c.uni((B, 1, max(1, H >> k), max(1, W >> k)), 0.0, 50.0)) for k in range(K)]
    lo = c.put(c.uni((B, 1, max(1, H >> K), max(1, W >> K)), 0.0, 30.0))
    hi = c.put(c.uni((B, 1, max(1, H >> K), max(1, W >> K)), 20.0, 50.0))
    return ops_deeppruner.deeppruner_final_maps(disps, lo, hi, (H, W))


def _forward(ops, c, name):
    m = DeepPruner(Config.fromfile(os.path.join(ROOT, R.CASES[name][0])))
    m.load_state_dict(R.model(name).state_dict(), strict=True)
    m = m.to(c.dev).eval()
    left, right, noise = R.inputs(name)
    with torch.no_grad():
        res, _ = m(dict(leftImage=c.put(left), rightImage=c.put(right), patchMatchNoise=c.put(noise)))
    return res["disps"]


_SHAPES = {
    "deeppruner_final_maps": (_tail, {"h4_w4_k3": (1, 4, 4, 3), "w24_b2_k1": (2, 8, 24, 1), "h16_w40_k3": (1, 16, 40, 3),
                                      "tiles_h24_w72_b2_k2": (2, 24, 72, 2)}),
    "DeepPruner": (_forward, {"8x_b2": ("8x",)}),
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
