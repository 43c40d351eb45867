"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; no unwritten output
word; results bit-identical to the plain run; 4-byte aligned operands) for the four wrappers of csrc/deeppruner_loss.hip:
``ops_deeppruner.deeppruner_loss_fwd`` / ``deeppruner_loss_bwd`` / ``quantile_loss_fwd`` / ``quantile_loss_bwd``.  The cases are
built here and run by that module's ``_run_case`` (both poison kinds, and the pass with operands 4 bytes off a 16-byte boundary);
the passes 8 and 12 bytes off are added below with the same helpers, as tests/test_memory_contract_deeppruner_model_gpu.py does.
That module's own table is not touched.

Shapes (B, H, W, K; the list at (H >> k, W >> k), the range maps at (H >> K, W >> K)): 4 x 4 down to 1 x 1 maps; B = 2 with 24
columns, less than one 64-column tile; odd quarter and eighth sizes; several tiles with a partial last one and B = 2.  The
forward's workspace and the counts come from the frame: a sum that read an unwritten workspace word would not equal the plain run."""
import pytest
import torch

from densematchingbenchmark_amd import ops_deeppruner
from tests.test_memory_contract_gpu import Case, Ctx, Frame, _check_framed, _execute, _run_case, _snapshot  # noqa: F401  (Ctx: the type a body receives)

pytestmark = pytest.mark.gpu
BOUNDS = (0.0, 192.0, 0.0, 192.0, 0.05)


def _maps(c, B, H, W, K):
    gt = c.uni((B, 1, H, W), -10.0, 230.0)
    gt[:, :, ::3, ::5] = 0.0
    sizes = [(max(1, H >> k), max(1, W >> k)) for k in range(K)]
    disps = [c.put(c.uni((B, 1) + s, 0.0, 200.0) * (s[1] / W)) for s in sizes]
    h, w = max(1, H >> K), max(1, W >> K)
    lo = c.put(c.uni((B, 1, h, w), 0.0, 150.0) * (w / W))
    hi = c.put(c.uni((B, 1, h, w), 50.0, 200.0) * (w / W))
    return disps, lo, hi, c.put(gt)


def _fused_fwd(ops, c, B, H, W, K):
    disps, lo, hi, gt = _maps(c, B, H, W, K)
    return list(ops_deeppruner.deeppruner_loss_fwd(disps, lo, hi, gt, *BOUNDS))


def _fused_bwd(ops, c, B, H, W, K):
    disps, lo, hi, gt = _maps(c, B, H, W, K)
    stats = c.put(torch.tensor([float(B * H * W - 7), float(B * H * W - 5)], dtype=torch.float64))
    go = c.put(c.uni((K + 4,), 0.5, 1.5))
    g_disps, g_lo, g_hi = ops_deeppruner.deeppruner_loss_bwd(disps, lo, hi, gt, stats, go, *BOUNDS)
    return g_disps + [g_lo, g_hi]


def _full(c, B, H, W):
    gt = c.uni((B, 1, H, W), -10.0, 230.0)
    gt[:, :, ::3, ::5] = 0.0
    return c.put(gt + c.rand((B, 1, H, W), 2.0) - 1.0), c.put(gt + c.rand((B, 1, H, W), 2.0) + 1.0), c.put(gt)


def _quantile_fwd(ops, c, B, H, W, K):
    lo, hi, gt = _full(c, B, H, W)
    return list(ops_deeppruner.quantile_loss_fwd(lo, hi, gt, 0.0, 192.0, 0.05))


def _quantile_bwd(ops, c, B, H, W, K):
    lo, hi, gt = _full(c, B, H, W)
    stats = c.put(torch.tensor([0.0, float(B * H * W - 5)], dtype=torch.float64))
    return list(ops_deeppruner.quantile_loss_bwd(lo, hi, gt, stats, c.put(c.uni((2,), 0.5, 1.5)), 0.0, 192.0, 0.05))


_CALLS = {"h4_w4_k3": (1, 4, 4, 3), "w24_b2_k1": (2, 8, 24, 1), "h16_w40_k3": (1, 16, 40, 3), "tiles_h24_w72_b2_k2": (2, 24, 72, 2)}
_SHAPES = {"deeppruner_loss_fwd": _fused_fwd, "deeppruner_loss_bwd": _fused_bwd, "quantile_loss_fwd": _quantile_fwd,
           "quantile_loss_bwd": _quantile_bwd}

CASES = [Case(_wrapper, "deeppruner", _label, _body, _args, "ok", False)
         for _wrapper, _body in _SHAPES.items() for _label, _args in _CALLS.items()]


@pytest.mark.parametrize("case", [pytest.param(k, id=k.id) for k in CASES])
def test_memory_contract(dev, case):
    _run_case(case, dev)
    for misalign in (8, 12):        # the frame's operands 8 and 12 bytes off a 16-byte boundary, against a plain run 4 bytes off
        c, res = _execute(case, dev, misalign=misalign)
        plain = _snapshot(c, res)
        for kind in ("nan", "huge"):
            _check_framed(case, dev, kind, misalign, plain)
