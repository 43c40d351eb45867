"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; no unwritten output
word; results bit-identical to the plain run; 4-byte aligned operands) for the two wrappers of the sampler's backward,
``ops.patch_match_step_bwd`` and ``ops.deeppruner_uniform_samples_bwd`` (defined in ``ops_deeppruner``, csrc/patch_match.hip).
The cases are built here and run by that module's ``_run_case`` (both poison kinds, and the pass with operands 4 bytes off a
16-byte boundary); the passes 8 and 12 bytes off are added below with the same helpers.  That module's own table is not touched.

The target-feature gradient of the step is summed in LDS in the hardware's order, as ``fast_fms_bwd``'s is, and is held to the
same stated exception (``AtomicOrder``: the FP64 rule); everything else, the workspace's consumers included, is bit-identical.
The workspace (gc, gn and the partial rows) is allocated inside the wrapper, so it starts poisoned and sits between guards.

Step shapes: W % 4 == 1 with B = 2 and C off the group of eight channels, the minimum 2 x 2 map with constants, a vertical step
with range maps and C = 33 (five channel groups, the last with one channel), and a map of several 256-pixel blocks with a partial
last one and more columns than a wave.  Uniform shapes: N = 2 (no inner sample), B = 2 with the range head, one row, several blocks."""
import pytest
import torch

from densematchingbenchmark_amd import ops_deeppruner
from tests import _deeppruner_ref as R
from tests.test_memory_contract_gpu import AtomicOrder, Case, Ctx, Frame, _check_framed, _execute, _run_case, _snapshot  # noqa: F401

pytestmark = pytest.mark.gpu


def _step_ref(left, right, noise, lo, hi, gS, gN, vertical, dtype):
    left, right, noise = (t.to(dtype).clone().requires_grad_() for t in (left, right, noise))
    s, n = R.half_iteration(left, right, noise, lo.to(dtype), hi.to(dtype), vertical)
    return torch.autograd.grad((s * gS.to(dtype)).sum() + (n * gN.to(dtype)).sum(), (left, right))


def _step_bwd(ops, c, shape, P, vertical, maps):
    B, C, H, W = shape
    left, right, noise = c.rand(shape), c.rand(shape), c.uni((B, P, H, W))
    gS, gN = c.rand((B, P, H, W)), c.rand((B, P, H, W))
    if maps:
        lo, hi = c.uni((B, 1, H, W), -3.0, 2.0), c.uni((B, 1, H, W), 0.5 * W, W + 3.0)
    else:
        lo, hi = torch.zeros((B, 1, H, W)), torch.full((B, 1, H, W), float(W))
    d = [c.put(t) for t in (left, right, noise)]
    rng = [c.put(lo), c.put(hi)] if maps else [None, None]
    dl, dr, dn = ops_deeppruner.patch_match_step_bwd(*d, *rng, grad_samples=c.put(gS), grad_noise=c.put(gN), vertical=vertical,
                                                     bounds=(0.0, float(W)))
    t64 = _step_ref(left, right, noise, lo, hi, gS, gN, vertical, torch.float64)
    t32 = _step_ref(left, right, noise, lo, hi, gS, gN, vertical, torch.float32)
    # a second call with only the noise's gradient and accumulators: dL keeps a fixed order, dR is covered above
    dl2, _, dn2 = ops_deeppruner.patch_match_step_bwd(*d, *rng, grad_noise=c.put(gN), vertical=vertical, bounds=(0.0, float(W)),
                                                      grad_left_acc=c.put(c.rand(shape)), grad_right_acc=c.put(c.rand(shape)))
    return [dl, AtomicOrder(dr, t64[1], t32[1]), dn, dl2, dn2]


def _uniform_bwd(ops, c, shape, N, max_disp):
    lo = c.put(c.uni(shape, -5.0, 30.0))
    hi = c.put(c.uni(shape, 2.0, 60.0))
    g = c.put(c.rand((shape[0], N) + tuple(shape[2:])))
    return list(ops_deeppruner.deeppruner_uniform_samples_bwd(lo, hi, g, max_disp))


_SHAPES = {
    "patch_match_step_bwd": (_step_bwd, {"w13_b2_c5": ((2, 5, 4, 13), 3, False, True), "h2_w2_consts": ((1, 8, 2, 2), 1, False, False),
                                         "c33_w7_vert": ((1, 33, 6, 7), 4, True, True), "blocks_w70": ((1, 4, 9, 70), 2, True, False)}),
    "deeppruner_uniform_samples_bwd": (_uniform_bwd, {"w13_n2": ((1, 1, 3, 13), 2, None), "w24_b2_n9_post": ((2, 1, 2, 24), 9, 48.0),
                                                      "h1_w22_n5_post": ((1, 1, 1, 22), 5, 24.0), "blocks_w70_n3": ((1, 1, 9, 70), 3, None)}),
}

CASES = [Case(_wrapper, "deeppruner_sampler_bwd", _label, _body, _args, "ok", False)
         for _wrapper, (_body, _calls) in _SHAPES.items() for _label, _args in _calls.items()]


@pytest.mark.parametrize("case", [pytest.param(k, id=k.id) for k in CASES])
def test_memory_contract(dev, case):
    _run_case(case, dev)
    for misalign in (8, 12):        # the frame's operands 8 and 12 bytes off a 16-byte boundary, against a plain run 4 bytes off
        c, res = _execute(case, dev, misalign=misalign)
        plain = _snapshot(c, res)
        for kind in ("nan", "huge"):
            _check_framed(case, dev, kind, misalign, plain)
