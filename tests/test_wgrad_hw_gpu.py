"""The weight gradient of the units that stride only height and width (stride (1, 2, 2): plan form 5 of dmb_conv_wgrad_plan,
csrc/wgrad.hip) alone, against torch's CPU autograd in FP64 and again in FP32:

    out[cs, cb, kz, ky, kx] = sum_{b, z, y, x} small[b, cs, z, y, x] * big[b, cb, z + kz - 1, 2y + ky - 1, 2x + kx - 1]

in both roles -- nn.Conv3d(k 3, s (1, 2, 2), p 1): small = dc, big = x; nn.ConvTranspose3d(k 3, s (1, 2, 2), p 1, output_padding
(0, 1, 1)): small = x, big = dy (an even big operand only) -- through ``ops.conv3d_k3s2_wgrad`` / ``ops.deconv3d_k3s2_wgrad``, which
pass the two shapes on unchanged.  The rule is that of tests/test_unit_grads_gpu.py: |hip - fp64| <= 4 |fp32 - fp64| + 2e-6 x range,
and a second call is bit-identical.

CASES: the smallest shapes at which the kernel can go wrong.  The form has two instantiations (16-byte and dword staging of the one
4 x 8 tile); each case asserts through the plan query which one it runs and how it is cut into segments on 256 compute units.  With
the fitted segment constants (a segment may be a single plane) "depth 14" runs as 14 one-plane segments; segments that walk the ring
and a shorter last one are what "deepest" (2, 2, 2, 2, 1) and "ring" (4, 3: every ring slot re-used) are there for."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_backward_gpu import _close

pytestmark = pytest.mark.gpu
HW = (1, 2, 2)
S2 = 2      # DMB_WGRAD_S2

# name: (small (B, Cs, D, H, W), big (Cb, D, Hb, Wb), plan code, (segment length, segments) at 256 compute units)
CASES = {
    "min_depth": ((2, 32, 2, 3, 5), (16, 2, 6, 10), 0x501, (1, 2)),          # the minimum depth, a partial tile on both axes
    "odd_big": ((2, 20, 5, 7, 13), (7, 5, 13, 25), 0x501, (1, 5)),           # odd big extents, partial channel blocks, dword staging
    "depth_14": ((1, 64, 14, 4, 12), (32, 14, 8, 24), 0x500, (1, 14)),       # the 16-byte path
    "deepest": ((1, 128, 9, 8, 16), (64, 9, 16, 32), 0x500, (2, 5)),         # the deepest training launch: 8 channel blocks share the slots
    "one_voxel": ((1, 40, 3, 1, 1), (33, 3, 1, 1), 0x501, (1, 3)),           # one voxel per plane
    "ring": ((2, 128, 7, 8, 32), (64, 7, 16, 64), 0x500, (4, 2)),            # segments of 4 + 3 planes: the ring of four wraps
}
ROLES = [(n, r) for n, c in CASES.items() for r in ("conv", "transposed") if r == "conv" or (c[1][2] % 2 == 0 and c[1][3] % 2 == 0)]


def _autograd(role, small, big, dtype):
    small, big = small.to(dtype), big.to(dtype)
    if role == "conv":      # small = dc, big = x
        w = torch.zeros((small.shape[1], big.shape[1], 3, 3, 3), dtype=dtype, requires_grad=True)
        F.conv3d(big, w, None, stride=HW, padding=1).backward(small)
    else:                   # small = x, big = dy
        w = torch.zeros((small.shape[1], big.shape[1], 3, 3, 3), dtype=dtype, requires_grad=True)
        F.conv_transpose3d(small, w, None, stride=HW, padding=1, output_padding=(0, 1, 1)).backward(big)
    return w.grad


@functools.lru_cache(maxsize=None)
def _data(name, role):
    """Operands (CPU, FP32) and the FP64 / FP32 autograd gradients of a case: computed once, never modified."""
    ss, sb, _, _ = CASES[name]
    g = torch.Generator().manual_seed(9100 + list(CASES).index(name))
    small, big = torch.randn(ss, generator=g), torch.randn((ss[0],) + sb, generator=g)
    return small, big, _autograd(role, small, big, torch.float64), _autograd(role, small, big, torch.float32)


def _run(ops, role, small, big):
    return ops.conv3d_k3s2_wgrad(big, small) if role == "conv" else ops.deconv3d_k3s2_wgrad(small, big)


def _off_by_4(t, dev):
    """A device copy of ``t`` that starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty((t.numel() + 1,), dtype=torch.float32, device=dev)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@pytest.mark.parametrize("name,role", ROLES, ids=["%s-%s" % nr for nr in ROLES])
def test_hw_weight_gradient_against_fp64_autograd(dev, name, role):
    from densematchingbenchmark_amd import ops
    _, _, code, segs = CASES[name]
    small, big, ref64, ref32 = _data(name, role)
    sd, bd = small.to(dev), big.to(dev)
    plan, detail = ops.conv_wgrad_plan(S2, sd, bd)
    assert (plan, detail[2:4]) == (code, segs), "%s: this device plans 0x%03x %s" % (name, plan, detail)
    got = _run(ops, role, sd, bd)
    assert got.shape == ref64.shape
    _close(got.cpu(), ref64, ref32, "%s %s (plan 0x%03x)" % (name, role, code))
    assert torch.equal(got, _run(ops, role, sd, bd)), "%s: the weight gradient must be bit-reproducible (no atomics)" % name


@pytest.mark.parametrize("role", ["conv", "transposed"])
def test_operands_4_bytes_off_a_16_byte_boundary(dev, role):
    """Rows of multiples of 4 floats, but neither operand aligned: the dword instantiation, the same numbers within the rule"""
    from densematchingbenchmark_amd import ops
    small, big, ref64, ref32 = _data("depth_14", role)
    sd, bd = _off_by_4(small, dev), _off_by_4(big, dev)
    assert ops.conv_wgrad_plan(S2, sd, bd)[0] == 0x501
    got = _run(ops, role, sd, bd)
    _close(got.cpu(), ref64, ref32, "depth_14 %s, misaligned" % role)
    assert torch.equal(got, _run(ops, role, sd, bd))


def test_one_plane_stays_on_the_stride_2_kernels(dev):
    """Ds == Db == 1 is the same sum in either reading and keeps its stride-2 plan (form 2)"""
    from densematchingbenchmark_amd import ops
    g = torch.Generator().manual_seed(9199)
    small, big = torch.randn((2, 32, 1, 5, 6), generator=g), torch.randn((2, 24, 1, 10, 12), generator=g)
    sd, bd = small.to(dev), big.to(dev)
    assert ops.conv_wgrad_plan(S2, sd, bd)[0] >> 8 == 2
    _close(_run(ops, "conv", sd, bd).cpu(), _autograd("conv", small, big, torch.float64), _autograd("conv", small, big, torch.float32),
           "one plane")
