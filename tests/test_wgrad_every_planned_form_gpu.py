"""Every instantiation the weight-gradient entry points can plan -- the 13 codes of dmb_conv_wgrad_plan (csrc/wgrad.hip) -- run at the
smallest launch found for it and compared with torch's FP64 autograd.

Which instantiation a launch takes follows its width class, the 16-byte alignment of its rows and, for the stride-2 tile, the
launch's SIZE against the slots its channel blocks leave: the shapes of tests/test_backward_gpu.py reach the forms as they happen to.
tests/test_wgrad_plan_host.py: GPU_CASES holds one shape per code with B = 2, two or more tiles, a PARTIAL last tile on every tiled
axis (the zero fill of the staging is what a tile can get wrong without a full volume noticing), a channel count off the multiples of
32 and, where the form walks segments, two or more with a shorter last one.

Per case: the plan of the launch about to be made (real alignments, this device's compute units) is the recorded one -- a device with
another CU count fails here by name instead of testing other kernels --; the result against FP64 autograd within ``_close`` of
tests/test_backward_gpu.py (4x the FP32 evaluation's own error plus 2e-6 of the range); a second call bit-identical (fixed-order
sums, no atomics); and, where one batch item alone plans the same code, the two single-item gradients add up to the batch's within
the same bound."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_backward_gpu import _close
from tests.test_wgrad_plan_host import D2, GPU_CASES, S2, gpu_case_shapes

pytestmark = pytest.mark.gpu
_BY_NAME = {c[0]: c for c in GPU_CASES}
_IDS = [c[0] for c in GPU_CASES]


def _ops():
    from densematchingbenchmark_amd import ops
    return ops


def _autograd(case, a, b, dtype):
    """The weight gradient by autograd of the forward convolution, evaluated in ``dtype`` on the CPU"""
    _, kind, Co, Ci, dims, k, dl, _, _ = case
    a, b = a.to(dtype), b.to(dtype)
    if kind == D2:
        w = torch.zeros((Co, Ci, k, k), dtype=dtype, requires_grad=True)
        F.conv2d(a, w, None, padding=dl * (k // 2), dilation=dl).backward(b)
    elif kind == S2:      # a = small = dc, b = big = x of nn.Conv3d(stride 2)
        w = torch.zeros((Co, Ci, 3, 3, 3), dtype=dtype, requires_grad=True)
        F.conv3d(b, w, None, stride=2, padding=1).backward(a)
    else:
        w = torch.zeros((Co, Ci, 3, 3, 3), dtype=dtype, requires_grad=True)
        F.conv3d(a, w, None, padding=1).backward(b)
    return w.grad


@functools.lru_cache(maxsize=None)
def _data(name):
    """The case's operands (CPU, FP32) and their FP64 / FP32 autograd gradients: computed once, never modified."""
    case = _BY_NAME[name]
    sa, sb = gpu_case_shapes(case)
    g = torch.Generator().manual_seed(7000 + _IDS.index(name))
    a, b = torch.randn(sa, generator=g), torch.randn(sb, generator=g)
    return a, b, _autograd(case, a, b, torch.float64), _autograd(case, a, b, torch.float32)


def _run(case, a, b):
    ops = _ops()
    _, kind, _, _, _, k, dl, _, _ = case
    if kind == D2:
        return ops.conv2d_wgrad(a, b, k, dl)
    return ops.conv3d_k3s2_wgrad(b, a) if kind == S2 else ops.conv3d_k3_wgrad(a, b)


@pytest.mark.parametrize("name", _IDS)
def test_every_planned_form_against_fp64_autograd(dev, name):
    ops = _ops()
    case = _BY_NAME[name]
    _, kind, Co, Ci, dims, k, dl, code, alone = case
    a, b, ref64, ref32 = _data(name)
    ad, bd = a.to(dev), b.to(dev)
    plan, detail = ops.conv_wgrad_plan(kind, ad, bd, k, dl)
    assert plan == code, "%s: this device plans 0x%03x %s, the case was recorded for 0x%03x at 256 compute units" % (name, plan, detail, code)
    got = _run(case, ad, bd)
    assert got.shape == ref64.shape
    _close(got.cpu(), ref64, ref32, "%s (plan 0x%03x)" % (name, code))
    assert torch.equal(got, _run(case, ad, bd)), "%s: the weight gradient must be bit-reproducible (no atomics)" % name
    if alone == code:
        ones = []
        for i in range(dims[0]):
            ai, bi = ad[i:i + 1].clone(), bd[i:i + 1].clone()      # (fresh allocations: 16-byte aligned like the batch)
            assert ops.conv_wgrad_plan(kind, ai, bi, k, dl)[0] == alone, "%s: item alone plans another code than recorded" % name
            ones.append(_run(case, ai, bi))
        _close((ones[0].double() + ones[1].double()).cpu(), ref64, ref32, "%s: sum of the batch items alone" % name)
