"""Every tile instantiation dmb_conv3d_k3_f32 can plan for a full-grid launch, run at its smallest launch and compared voxel by
voxel with an FP64 convolution.

Which tile a stride-1 or stride-2 launch takes is a cost estimate over workgroup rounds (csrc/conv3d_s1s2.hip): a launch that fits
one round on 256 compute units gets the smallest tile whatever its width, so the small shapes of tests/test_kernels_gpu.py and
tests/test_fuzz_gpu.py run the smallest tiles and split-K, and the large tiles were seen through whole-model outputs only, at
shapes they divide exactly.  tests/test_conv3d_plan_host.py: GPU_CASES holds, per plan code, the smallest shape that reaches the
code with two or more tiles and a PARTIAL last tile along x, y and z of that tile -- the zero fill of the staging and the masks of
the epilogue are what a tile can get wrong without a full volume noticing.

Per case: the plan of the launch about to be made (real alignments, this device's compute units) is the recorded one -- a device
with another CU count fails here by name instead of testing other tiles --; plain, folded affine + skip + ReLU, and ReLU-then-skip,
each into a fresh tensor and into the caller's ``out=`` (pre-filled with NaN), against F.conv3d in FP64 on the CPU: unit-variance
inputs, weights scaled by 1 / sqrt(27 Ci), so outputs are O(1) and the bound is the project's 2e-5 for one such layer
(tests/test_kernels_gpu.py; F.conv3d in FP32 on the CPU is 2.7e-6 .. 3.2e-6 from the same FP64 values at the three largest
cases).  A failure names the worst output's (b, c, z, y, x) and where it sits inside its tile.

Under the single-chain flag every batch item run alone -- another plan, asserted, wherever the list has a smaller tile -- is
bit-identical to its slice of the batched result: include/dmb_hip.h promises ONE k-ordered fma chain per output for every
full-grid form, whatever the tile.  The 32-channel stride-1 tiles also run as dmb_conv3d_k3_bnstats_f32: the raw output bit for
bit, exactly dmb_conv3d_k3_bnstats_partials slots, and mean / variance finished from the partial sums against FP64 statistics of
the FP64 convolution.

Checked by hand when the module was written (not repeated here): the stride-1 epilogue's result scaled by (1 + 2^-12) on the last
tile-local row of the 24 x 8 tile -- values only, no address, bound or launch geometry -- failed the three tests here on
s1_32_24x8 and s1_32_24x8_ci33 (2.4e-4 of the value, "y = 7 inside its 24 x 8 x 4 tile") while tests/test_kernels_gpu.py and
tests/test_fuzz_gpu.py passed all 297 cases: neither runs that tile.  On an MI355X the module takes about 5 s, the slowest case
0.4 s; the largest error over all cases is 1.25e-5 (s1_64_32x4 with affine and skip operand)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv3d_plan_host import GPU_CASES, TILES

pytestmark = pytest.mark.gpu
BOUND = 2e-5
_BY_NAME = {c[0]: c for c in GPU_CASES}
_IDS = [c[0] for c in GPU_CASES]
MODES = {"plain": (False, False, False), "skip_relu": (True, True, True), "relu_then_skip": (True, True, "pre")}   # affine, skip, relu


def _ops():
    from densematchingbenchmark_amd import ops
    return ops


def _affine(C, seed):     # (as tests/test_kernels_gpu.py: a folded BatchNorm with scale in [0.5, 1.5) and shift in [-0.5, 0.5))
    g = torch.Generator().manual_seed(seed)
    return 0.5 + torch.rand(C, generator=g), torch.rand(C, generator=g) - 0.5


@functools.lru_cache(maxsize=None)
def _data(name):
    """The case's operands (CPU, FP32) and the FP64 convolution of them: computed once, shared by the tests below, never modified."""
    _, Ci, Co, stride, (B, D, H, W), _, _, _ = _BY_NAME[name]
    g = torch.Generator().manual_seed(1000 + _IDS.index(name))
    x = torch.randn((B, Ci, D, H, W), generator=g)
    w = torch.randn((Co, Ci, 3, 3, 3), generator=g) / math.sqrt(27 * Ci)
    sc, sh = _affine(Co, 2000 + _IDS.index(name))
    conv = F.conv3d(x.double(), w.double(), None, stride=stride, padding=1)
    res = torch.randn(conv.shape, generator=g)
    return x, w, sc, sh, res, conv


def _expected(name, mode):
    _, _, sc, sh, res, conv = _data(name)
    affine, skip, relu = MODES[mode]
    ref = conv * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1) if affine else conv
    if relu == "pre":
        ref = F.relu(ref)
    if skip:
        ref = ref + res.double()
    return F.relu(ref) if relu is True else ref


def _out_tensor(shape, shift, dev):
    """A caller's output filled with NaN; ``shift`` floats off the allocator's 16-byte alignment."""
    n = math.prod(shape)
    return torch.full((n + shift,), float("nan"), device=dev)[shift:].view(shape)


def _where(code, stride, W, idx):
    """'(b, c, z, y, x), tile-local ...' of a flat output index, for the failure message."""
    b, c, z, y, x = idx
    t = TILES[code]
    if t == "runs":
        return "(b, c, z, y, x) = %s, voxel %d of its 64-voxel run, z-slice %d of 2" % (idx, (y * W + x) % 64, z % 2)
    return "(b, c, z, y, x) = %s, (x, y, z) = (%d, %d, %d) inside its %d x %d x %d tile" % (idx, x % t[0], y % t[1], z % t[2], t[0], t[1], t[2])


def _assert_close(got, ref, code, stride, what):
    err = (got.double().cpu() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)     # an unwritten (NaN) output is the worst one
    worst = err.max().item()
    print("%s: max |hip - fp64| = %.3g" % (what, worst))
    if worst > BOUND:
        idx = tuple(int(v) for v in torch.unravel_index(err.argmax(), err.shape))
        n_bad = int((err > BOUND).sum())
        raise AssertionError("%s (plan 0x%03x): |hip - fp64| = %g > %g at %s: got %r, expected %r; %d of %d outputs beyond the bound" % (
            what, code, worst, BOUND, _where(code, stride, err.shape[-1], idx), got[idx].item(), ref[idx].item(), n_bad, err.numel()))


@pytest.mark.parametrize("name", _IDS)
def test_every_planned_form_against_fp64(dev, name):
    ops = _ops()
    _, Ci, Co, stride, shape, code, _, shift = _BY_NAME[name]
    x, w, sc, sh, res, conv = _data(name)
    xd, scd, shd, resd = x.to(dev), sc.to(dev), sh.to(dev), res.to(dev)
    wp = ops.pack_conv3d_weights(w.to(dev))
    for mode, (affine, skip, relu) in MODES.items():
        ref = _expected(name, mode)
        args = (scd if affine else None, shd if affine else None, resd if skip else None)
        for into in ("fresh", "out"):
            if into == "fresh" and shift:
                continue     # (this case's code is the one a 4-byte aligned output selects)
            out = None if into == "fresh" else _out_tensor(tuple(conv.shape), shift, dev)
            # first: this launch, on this device, is the instantiation the case is there for
            plan = ops.conv3d_k3_plan(xd, Co, stride, args[2], out)
            assert plan == code, "%s: this device plans 0x%03x for the launch, the case was recorded for 0x%03x at 256 compute units" % (name, plan, code)
            got = ops.conv3d_k3(xd, wp, Co, *args, stride=stride, relu=relu, out=out)
            assert out is None or got.data_ptr() == out.data_ptr()
            _assert_close(got, ref, code, stride, "%s %s %s" % (name, mode, into))


@pytest.mark.parametrize("name", _IDS)
@pytest.mark.usefixtures("single_chain")
def test_batch_item_alone_is_bit_identical(dev, name):
    ops = _ops()
    _, Ci, Co, stride, shape, code, alone, shift = _BY_NAME[name]
    x, w, sc, sh, res, conv = _data(name)
    xd, scd, shd, resd = x.to(dev), sc.to(dev), sh.to(dev), res.to(dev)
    wp = ops.pack_conv3d_weights(w.to(dev))
    out = _out_tensor(tuple(conv.shape), shift, dev)
    assert ops.conv3d_k3_plan(xd, Co, stride, resd, out) == code
    both = ops.conv3d_k3(xd, wp, Co, scd, shd, resd, stride, True, out=out)
    for b in range(shape[0]):
        xb, rb = xd[b:b + 1].clone(), resd[b:b + 1].clone()      # (fresh allocations: 16-byte aligned like the batch)
        ob = _out_tensor((1,) + tuple(conv.shape[1:]), shift, dev)
        assert ops.conv3d_k3_plan(xb, Co, stride, rb, ob) == alone, "%s: item alone plans another code than recorded" % name
        one = ops.conv3d_k3(xb, wp, Co, scd, shd, rb, stride, True, out=ob)
        if not torch.equal(one[0], both[b]):
            diff = (one[0] != both[b])
            idx = (b,) + tuple(int(v) for v in torch.unravel_index(diff.int().argmax(), diff.shape))
            raise AssertionError("%s: batch item %d alone (plan 0x%03x) differs from its slice of the batch (plan 0x%03x) in %d outputs, first at %s" % (
                name, b, alone, code, int(diff.sum()), _where(code, stride, both.shape[-1], idx)))


_STATS = [c[0] for c in GPU_CASES if c[5] in (0x200, 0x201, 0x202, 0x203)]


@pytest.mark.parametrize("name", _STATS)
@pytest.mark.usefixtures("single_chain")
def test_statistics_launch_on_every_32_channel_tile(dev, name):
    ops = _ops()
    from densematchingbenchmark_amd import _lib
    _, Ci, Co, stride, (B, D, H, W), code, _, _ = _BY_NAME[name]
    x, w, _, _, _, conv = _data(name)
    xd = x.to(dev)
    wp = ops.pack_conv3d_weights(w.to(dev))
    assert ops.conv3d_k3_plan(xd, Co) == code
    fused = ops.conv3d_k3_bnstats(xd, wp, Co)
    assert fused is not None
    raw, parts = fused
    tx, ty, tz = TILES[code]
    slots = B * -(-W // tx) * -(-H // ty) * -(-D // tz)
    assert tuple(parts.shape) == (Co, slots, 2) and slots == _lib.load().dmb_conv3d_k3_bnstats_partials(B, Ci, Co, D, H, W)
    assert torch.equal(raw, ops.conv3d_k3(xd, wp, Co))
    _assert_close(raw, conv, code, 1, "%s statistics launch, raw output" % name)
    n = B * D * H * W
    tot = parts.cpu().sum(dim=1)
    mean, ref_mean = tot[:, 0] / n, conv.mean(dim=(0, 2, 3, 4))
    var, ref_var = tot[:, 1] / n - mean * mean, conv.var(dim=(0, 2, 3, 4), unbiased=False)
    # tests/test_backward_gpu.py, test_batch_statistics_from_the_convolution_epilogue: 1e-6 relative + 2e-7
    for got, ref, what in ((mean, ref_mean, "mean"), (var, ref_var, "variance")):
        err, tol = (got - ref).abs().max().item(), 1e-6 * max(1.0, ref.abs().max().item()) + 2e-7
        print("%s %s: max error %.3g (tolerance %.3g)" % (name, what, err, tol))
        assert err <= tol, "%s: %s from the partial sums is %g from the FP64 statistics (tolerance %g)" % (name, what, err, tol)
