"""Every form the up-sampling and regression entry points can plan (csrc/upsample_plan.h: the 24 forward codes of dmb_upsample_plan, the
4 adjoint codes of dmb_upsample_bwd_plan), each run at a launch found with the query for THIS device's compute units, and every
sampling-ratio class -- one input position, one output position, in == out, up- and down-sampling -- on every axis, against
F.interpolate(align_corners=True) on the CPU.

Forward, per case: ATen FP32 within the suite's 2e-6; ATen FP64 within max(2e-6, 2 x max |ATen FP32 - FP64|) of that case (the factor
2: two FP32 evaluations of the same weights may differ by their fma contraction); two forms of one entry on the same items (a batch
and its items alone, fused and unfused, one and four columns per thread, every zsplit) bit for bit; the fused disparity bit for bit
soft_argmin(y); soft_argmin against the FP64 oracle within 2e-5 max(1, D / 64).
Adjoints: FP64 autograd of F.interpolate (and of the softmax regression on it) within max(2e-6, 2 x max |ATen FP32 autograd - FP64|)
of that case and gradient -- the forward's rule, for the regression's gradient too although its kernel takes __expf and another
summation order than ATen; the tolerance never exceeds the Wo / 100-scaled bounds of
tests/test_backward_gpu.py::test_upsample_regression_backward, which is asserted.  The dot-product identity <A x, g> = <x, A^T g>
with the GPU forward and the GPU adjoint, sums in FP64 on the host, per batch item, relative to |A x| |g|: within 2 x the largest gap
the same identity leaves with ATen's FP32 forward and autograd over 32 probes of the case's shape (one probe's gap is a random sum
that can be zero by luck; the largest of 32 is a scale), and never below IDENTITY_FLOOR, the rounding of the host's own FP64 sums:
where every weight is 0 or 1 (in == out, integer down-sampling ratios) both operators are exact and both gaps are that noise.

Largest values measured on an MI355X (256 compute units): |GPU - ATen FP32| 4.8e-7; FP64 tolerance 1.07e-5 (|GPU - FP64| 5.4e-6 there);
adjoints 2.5e-4 under a tolerance of 5.1e-4 on gradients of magnitude 40, never above 0.62 of the case's tolerance; identity gap
2.3e-8 -- in full under MEASURED below.

The module runs whole and in file order in one process: test_every_form_was_run, last, reads what the tests before it launched, so
a -k selection, a random order or a split over workers fails it."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import dmb_oracle as O
from tests.test_upsample_plan_host import (AC, AC_SA, B_AC, B_AC_SA, B_BIL, BWD_REACHABLE, K8, K8_SA, REACHABLE, ROWS, SA, VOXEL_LOOP,
                                           VOXEL_WINDOW, WAVE, bwd_plan, plan)

pytestmark = pytest.mark.gpu

# Measured on an MI355X (256 compute units), the largest over the module's cases; each test prints its own figures with -s.
#   forward:      |GPU - ATen FP32| 4.8e-7 (bound 2e-6);  |GPU - FP64| 5.4e-6 where the tolerance max(2e-6, 2 |ATen FP32 - FP64|) is 1.07e-5,
#                 its largest value (1200 and 1600 output columns); |GPU - FP64| never above 0.54 of the case's tolerance
#   k8 / s4:      |GPU - ATen FP32| 0;  |GPU - FP64| 1.7e-7 (tolerance 2e-6)
#   soft-argmin:  |disp - FP64| 7.6e-6 at 256 planes (bound 8e-5), never above 0.10 of the bound
#   adjoints:     tolerance max(2e-6, 2 |ATen FP32 autograd - FP64|) per case and gradient.  Interpolation 2.4e-4 (4.7e-4: 1200 columns,
#                 gradients of magnitude 40); regression 6.5e-5 (3.8e-4: 256 planes); both in one call 2.5e-4 (5.1e-4); 2-D entry 1.6e-4
#                 (3.3e-4); one wave per input 1.9e-5 (2.2e-4).  |error| / tolerance at most 0.62 (interpolation, 1.2e-6 of 2e-6), 0.51
#                 (regression), 0.57 (both), 0.58 (2-D entry): the kernels' errors are ATen FP32's own, as the shared weights make them
#   identity:     relative gap 2.3e-8 at most, never above 0.65 of 2 x ATen's largest of 32 probes; exactly 0 (or the 1e-17 of the FP64 sums) where all weights
#                 are 0 or 1
MEASURED = {"forward_vs_aten_fp32": 4.77e-07, "forward_vs_fp64": 5.36e-06, "forward_fp64_tolerance": 1.07e-05, "soft_argmin_vs_fp64": 7.58e-06,
            "adjoint_vs_fp64": 2.46e-04, "adjoint_tolerance": 5.07e-04, "adjoint_worst_share_of_tolerance": 0.62, "identity_gap": 2.33e-08}

CAP_BYTES = 64 << 20
# FP64 sums of up to 2^23 products: about sqrt(N) 2^-53 = 3e-13 relative to the sum of magnitudes; four orders below the FP32 gaps (1e-8)
IDENTITY_FLOOR = 1e-12
RAN, RAN_BWD = set(), set()


def _ops():
    from densematchingbenchmark_amd import ops
    return ops


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _this(entry, B, i, o):
    """The plan of this launch on this device: (code, (columns per thread, flat, zsplit, grid x, y, z, threads))."""
    code, detail, why = plan(entry, B, i, o, 0)
    assert code > 0, (entry, B, i, o, why)
    return code, detail


def _interp(x, size, dtype):
    return F.interpolate(x.to(dtype).unsqueeze(1), size=list(size), mode="trilinear", align_corners=True).squeeze(1)


def _tol(ref32, ref64):
    """The tolerance against FP64 that the reference alone gives: twice ATen FP32's own error, 2e-6 at the least."""
    return max(2e-6, 2 * (ref32.double() - ref64).abs().max().item())


def _check_forward(got, x, size, what):
    """got (CPU) against ATen FP32 and FP64; returns the FP64 tolerance."""
    r32, r64 = _interp(x, size, torch.float32), _interp(x, size, torch.float64)
    e32 = (got - r32).abs().max().item()
    tol = _tol(r32, r64)
    e64 = (got.double() - r64).abs().max().item()
    print("%s: |GPU - ATen FP32| %.3g (2e-6), |GPU - FP64| %.3g (tolerance %.3g)" % (what, e32, e64, tol))
    assert tol <= 1e-5 * max(1.0, size[2] / 100.0) * max(1.0, r64.abs().max().item()), what
    assert e32 <= 2e-6, what
    assert e64 <= tol, what
    return tol


def _check_regression(disp, y, vals, what):
    """disp against the FP64 soft-argmin of the volume y the same launch (or its unfused twin) wrote."""
    D = len(vals)
    truth = O.soft_argmin_f64(y.cpu(), D)
    err = (disp.cpu().double() - truth).abs().max().item()
    print("%s: |disp - FP64 soft-argmin| %.3g (%.3g)" % (what, err, 2e-5 * max(1.0, D / 64)))
    assert err <= 2e-5 * max(1.0, D / 64), what


def _grow(entry, i, o, want, start=1):
    """Double the batch until the plan of [B, *i] -> o on this device satisfies ``want(code, detail)``; the output stays under the cap."""
    B = start
    while B * o[0] * o[1] * o[2] * 4 <= CAP_BYTES:
        code, detail = _this(entry, B, i, o)
        if want(code, detail):
            return B, code, detail
        B *= 2
    return None


# ------------------------------------------------------------------------------------------------------------ forward forms
@pytest.mark.parametrize("Wo", [64, 62], ids=["flat", "row"])
def test_fused_four_and_one_column_and_unfused_agree(dev, Wo):
    """[B, 3, 16, 16] -> (9, 64, Wo): the batch grown until the fused entry plans four columns per thread; each item alone takes one
    column; the unfused entry runs the batch and the items with whatever plane split the query names.  All bit for bit."""
    ops = _ops()
    i, o = (3, 16, 16), (9, 64, Wo)
    found = _grow(AC_SA, i, o, lambda code, d: d[0] == 4)
    assert found, "four columns per thread not reached under %d MiB" % (CAP_BYTES >> 20)
    B, code4, d4 = found
    code1, d1 = _this(AC_SA, 1, i, o)
    assert d1[0] == 1 and d4[1] == d1[1] == (Wo % 4 == 0), (d1, d4)
    x = _rand((B,) + i, 31)
    xd = x.to(dev)
    vals = ops.disp_sample_values(9, 0, 1)
    y4, disp4 = ops.trilinear_ac_soft_argmin(xd, o, vals, 1.0)
    RAN.add(code4)
    _check_forward(y4.cpu(), x, o, "fused, four columns, B = %d (0x%x)" % (B, code4))
    assert torch.equal(disp4, ops.soft_argmin(y4, vals, 1.0, True))
    _check_regression(disp4, y4, vals, "fused, four columns")
    ucode, ud = _this(AC, B, i, o)
    yu = ops.trilinear_ac(xd, o)
    RAN.add(ucode)
    assert torch.equal(yu, y4), "unfused (0x%x) against fused (0x%x)" % (ucode, code4)
    ucode1, ud1 = _this(AC, 1, i, o)
    for b in range(B):
        xb = xd[b:b + 1].clone()
        y1, disp1 = ops.trilinear_ac_soft_argmin(xb, o, vals, 1.0)
        assert torch.equal(y1[0], y4[b]) and torch.equal(disp1[0], disp4[b]), "item %d alone (0x%x) against the batch (0x%x)" % (b, code1, code4)
        assert torch.equal(ops.trilinear_ac(xb, o)[0], y4[b]), "item %d alone, unfused (0x%x)" % (b, ucode1)
    RAN.update((code1, ucode1))
    # the volume-free kernel: identical logits, another grouping of the max-rescale (tests/test_kernels_gpu.py: 2e-5)
    pcode, _ = _this(SA, B, i, o)
    dp = ops.trilinear_soft_argmin(xd, o, vals, 1.0)
    RAN.add(pcode)
    assert (dp - disp4).abs().max().item() <= 2e-5
    _check_regression(dp, y4, vals, "volume-free pixel kernel")


@pytest.mark.parametrize("zsplit", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("Wo", [64, 62], ids=["flat", "row"])
def test_unfused_every_plane_split(dev, Wo, zsplit):
    """[B, 3, 16, 16] -> (Do, 64, Wo) with the batch (and, for the split the 9 planes cannot reach, the plane count) chosen by the
    query so that the walk over the planes is cut in ``zsplit`` parts; against ATen, and bit for bit against each item alone, which
    the query gives another split."""
    ops = _ops()
    i = (3, 16, 16)
    found = None
    for Do in (9, 17, 5, 3):
        got = _grow(AC, i, (Do, 64, Wo), lambda code, d: d[2] == zsplit)
        if got and (found is None or got[0] * Do < found[1][0] * found[0]):
            found = (Do, got)
    assert found, "zsplit %d not reached under %d MiB" % (zsplit, CAP_BYTES >> 20)
    Do, (B, code, d) = found
    o = (Do, 64, Wo)
    assert code == 0x100 + (8 if Wo % 4 == 0 else 0) + zsplit.bit_length() - 1
    x = _rand((B,) + i, 32)
    xd = x.to(dev)
    y = ops.trilinear_ac(xd, o)
    RAN.add(code)
    _check_forward(y.cpu(), x, o, "unfused 0x%x: B = %d, %d planes in %d parts" % (code, B, Do, zsplit))
    code1, d1 = _this(AC, 1, i, o)
    alone = torch.cat([ops.trilinear_ac(xd[b:b + 1].clone(), o) for b in range(B)])
    RAN.add(code1)
    assert torch.equal(alone, y), "0x%x against the items alone (0x%x)" % (code, code1)
    if Do <= 9:      # the fused walk is never split
        yf, _ = ops.trilinear_ac_soft_argmin(xd, o, ops.disp_sample_values(Do, 0, 1), 1.0)
        assert torch.equal(yf, y)


def test_trilinear_past_65535_rows(dev):
    """[1, 2, 3, 2] -> (3, 65536, 5): more rows than grid y holds take the kernel with one thread per four outputs of a row."""
    ops = _ops()
    i, o = (2, 3, 2), (3, 65536, 5)
    code, d = _this(AC, 1, i, o)
    assert code == 0x200
    x = _rand((1,) + i, 33)
    y = ops.trilinear_ac(x.to(dev), o)
    RAN.add(code)
    _check_forward(y.cpu(), x, o, "rows past grid y")
    # a row both kernels can run: one row fewer takes the z-column kernel with other weights, but output row 0 is input row 0 (source
    # coordinate 0, weights 1 and 0) whatever the height
    y2 = ops.trilinear_ac(x.to(dev), (3, 65535, 5))
    assert _this(AC, 1, i, (3, 65535, 5))[0] >> 8 == 1 and torch.equal(y2[:, :, 0], y[:, :, 0])


@pytest.mark.parametrize("with_disp", [False, True], ids=["volume", "regression"])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 129, 256, 257])
def test_k8s4_every_workgroup_size(dev, W, with_disp):
    ops = _ops()
    B, D, H = 2, 2, 2
    code, d = _this(K8_SA if with_disp else K8, B, (D, H, W), (4 * D, 4 * H, 4 * W))
    nwg = -(-W // 256)
    threads = -(-(-(-W // nwg)) // 64) * 64          # a workgroup's share of the row, in whole waves
    assert d[3:] == (nwg, 4 * H, B, threads) and code == 0x500 + (4 if with_disp else 0) + threads // 64 - 1
    x, w = _rand((B, D, H, W), 34), _rand((8, 8, 8), 35, 0.1)
    vals = ops.disp_sample_values(4 * D, 0, 1)
    y, disp = ops.deconv3d_k8s4_c1_soft_argmin(x.to(dev), w.to(dev), vals if with_disp else None, 1.0)
    RAN.add(code)
    r32 = F.conv_transpose3d(x.unsqueeze(1), w.view(1, 1, 8, 8, 8), None, stride=4, padding=2).squeeze(1)
    r64 = F.conv_transpose3d(x.double().unsqueeze(1), w.double().view(1, 1, 8, 8, 8), None, stride=4, padding=2).squeeze(1)
    tol = _tol(r32, r64)
    e32, e64 = (y.cpu() - r32).abs().max().item(), (y.cpu().double() - r64).abs().max().item()
    print("k8s4 W = %d (0x%x): |GPU - ATen FP32| %.3g (1e-5), |GPU - FP64| %.3g (tolerance %.3g)" % (W, code, e32, e64, tol))
    assert y.shape == r32.shape and e32 <= 1e-5 and e64 <= tol
    assert torch.equal(y, ops.deconv3d_k8s4_c1(x.to(dev), w.to(dev))), "the z-column walk against the one-thread-per-row-word kernel"
    if with_disp:
        assert (disp is not None) and torch.equal(disp, ops.soft_argmin(y, vals, 1.0, True))
        _check_regression(disp, y, vals, "k8s4 + regression")
    else:
        assert disp is None


@pytest.mark.parametrize("Do", [1, 7, 8, 9, 256])
def test_fused_plane_counts(dev, Do):
    """One plane, a tail only, one block of 8, a block and a tail, the largest sample count -- up- and (Di = 12, Do < 12) down-sampled --
    through the fused forward entries and the fused adjoint, whose z kernel walks the planes with a softmax of its own."""
    ops = _ops()
    i, o = (12, 5, 7), (Do, 9, 14)
    x = _rand((2,) + i, 36)
    vals = ops.disp_sample_values(Do, 0, 1)
    code, _ = _this(AC_SA, 2, i, o)
    y, disp = ops.trilinear_ac_soft_argmin(x.to(dev), o, vals, 1.0)
    RAN.add(code)
    _check_forward(y.cpu(), x, o, "fused, %d planes" % Do)
    assert torch.equal(y, ops.trilinear_ac(x.to(dev), o)) and torch.equal(disp, ops.soft_argmin(y, vals, 1.0, True))
    _check_regression(disp, y, vals, "fused, %d planes" % Do)
    dp = ops.trilinear_soft_argmin(x.to(dev), o, vals, 1.0)
    assert (dp - disp).abs().max().item() <= 2e-5 * max(1.0, Do / 64)
    _check_adjoints(dev, i, o, 40 + Do, "adjoints, %d planes" % Do)


def test_fused_entries_refuse_257_planes(dev):
    from densematchingbenchmark_amd import _lib
    ops = _ops()
    x = _rand((1, 3, 4, 6), 37).to(dev)
    vals = [float(k) for k in range(257)]
    for entry in (AC_SA, SA):
        assert plan(entry, 1, (3, 4, 6), (257, 8, 12), 0)[0] == -100001
    with pytest.raises(_lib.DmbLibraryError):
        ops.trilinear_ac_soft_argmin(x, (257, 8, 12), vals, 1.0)
    with pytest.raises(_lib.DmbLibraryError, match="disparity sample count out of range"):
        ops.trilinear_soft_argmin(x, (257, 8, 12), vals, 1.0)
    with pytest.raises(_lib.DmbLibraryError, match="disparity sample count out of range"):
        ops.trilinear_ac_soft_argmin_bwd(x, x, x, (257, 8, 12), vals, 1.0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ adjoints
@functools.lru_cache(maxsize=None)
def _aten_identity_gap(i, o):
    """The largest relative gap |<A x, g> - <x, A^T g>| / (|A x| |g|) over 32 probes with ATen's FP32 forward and autograd (sums in FP64)."""
    x = _rand((32,) + i, 41).requires_grad_(True)
    g = _rand((32,) + o, 42)
    y = _interp(x, o, torch.float32)
    gx, = torch.autograd.grad(y, x, g)
    return max(_gaps(x.detach(), y.detach(), g, gx).max().item(), IDENTITY_FLOOR / 2)


def _gaps(x, y, g, gx):
    x, y, g, gx = (t.double().flatten(1) for t in (x, y, g, gx))
    return ((y * g).sum(1) - (x * gx).sum(1)).abs() / (y.norm(dim=1) * g.norm(dim=1)).clamp_min(1e-300)


@functools.lru_cache(maxsize=None)
def _adjoint_reference(i, o, seed):
    """Operands (CPU FP32, never modified) and the FP64 / ATen FP32 autograd gradients of [2, *i] -> o: of a gradient gv on the volume, of
    a gradient g on the regressed disparity and of both at once, with their tolerances."""
    Do, Ho, Wo = o
    x, gv, g = _rand((2,) + i, seed, 2.0), _rand((2,) + o, seed + 1), _rand((2, 1, Ho, Wo), seed + 2)
    vals = O.disp_sample_values(Do).tolist()
    out = {}
    for dtype in (torch.float64, torch.float32):
        xr = x.to(dtype).requires_grad_(True)
        up = _interp(xr, o, dtype)
        disp = (torch.softmax(up, dim=1) * torch.tensor(vals, dtype=dtype).view(1, Do, 1, 1)).sum(1, keepdim=True)
        rv, = torch.autograd.grad(up, xr, gv.to(dtype), retain_graph=True)
        rd, = torch.autograd.grad(disp, xr, g.to(dtype), retain_graph=True)
        rb, = torch.autograd.grad([up, disp], xr, [gv.to(dtype), g.to(dtype)])
        out[dtype] = (rv, rd, rb)
    (rv, rd, rb), r32 = out[torch.float64], out[torch.float32]
    wide = max(1.0, Wo / 100.0)
    tol_v, tol_d, tol_b = (_tol(a32, a) for a32, a in zip(r32, (rv, rd, rb)))
    assert tol_v <= 1e-5 * wide * max(1.0, rv.abs().max().item()) and tol_d <= 5e-5 * wide * max(1.0, rd.abs().max().item())
    assert tol_b <= 5e-5 * wide * max(1.0, rb.abs().max().item())
    return x, gv, g, vals, rv, rd, rb, tol_v, tol_d, tol_b


def _check_adjoints(dev, i, o, seed, what, want=None):
    """The three adjoint entries on [2, *i] -> o; ``want``: the form the trilinear entries must plan."""
    ops = _ops()
    (Di, Hi, Wi), (Do, Ho, Wo) = i, o
    x, gv, g, vals, rv, rd, rb, tol_v, tol_d, tol_b = _adjoint_reference(i, o, seed)
    xd, gvd, gd = x.to(dev), gv.to(dev), g.to(dev)
    code, detail, why = bwd_plan(B_AC, 2, Di, (Hi, Wi), Do, (Ho, Wo), 0)
    assert code > 0 and bwd_plan(B_AC_SA, 2, Di, (Hi, Wi), Do, (Ho, Wo), 0)[:2] == (code, detail), why
    assert want is None or code == want, "%s plans form %d %s, not %d" % (what, code, detail, want)
    # the interpolation's adjoint
    gotv = ops.trilinear_ac_bwd(gvd, i)
    ev = (gotv.cpu().double() - rv).abs().max().item()
    # the regression's, alone and with the volume's
    y, disp = ops.trilinear_ac_soft_argmin(xd, o, vals, 1.0)
    gotd = ops.trilinear_ac_soft_argmin_bwd(xd, disp, gd, o, vals, 1.0)
    both = ops.trilinear_ac_soft_argmin_bwd(xd, disp, gd, o, vals, 1.0, grad_cost=gvd)
    RAN_BWD.add(code)
    ed = (gotd.cpu().double() - rd).abs().max().item()
    eb = (both.cpu().double() - rb).abs().max().item()
    # <A x, g> = <x, A^T g> with the GPU's forward and adjoint
    gap = _gaps(x, y.cpu(), gv, gotv.cpu()).max().item()
    gap_tol = 2 * _aten_identity_gap(i, o)
    print("%s (form %d): interpolation adjoint %.3g (%.3g), regression %.3g (%.3g) and with the volume's %.3g (%.3g), identity %.3g (%.3g)"
          % (what, code, ev, tol_v, ed, tol_d, eb, tol_b, gap, gap_tol))
    assert gotv.shape == x.shape and ev <= tol_v, what
    assert ed <= tol_d and eb <= tol_b, what
    assert gap <= gap_tol, what
    # the 2-D entry on the same planes: channels = Di
    code2, detail2, why = bwd_plan(B_BIL, 2, Di, (Hi, Wi), 0, (Ho, Wo), 0)
    assert code2 > 0, why
    g2 = gv[:, :Di].contiguous() if Do >= Di else _rand((2, Di, Ho, Wo), seed + 3)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        xr = x.to(dtype).requires_grad_(True)
        refs[dtype], = torch.autograd.grad(F.interpolate(xr, size=[Ho, Wo], mode="bilinear", align_corners=True), xr, g2.to(dtype))
    r2 = refs[torch.float64]
    tol2 = _tol(refs[torch.float32], r2)
    got2 = ops.bilinear_ac_bwd(g2.to(dev), (Hi, Wi))
    RAN_BWD.add(code2)
    e2 = (got2.cpu().double() - r2).abs().max().item()
    gap2 = _gaps(x, ops.bilinear_ac(xd, (Ho, Wo)).cpu(), g2, got2.cpu()).max().item()
    gap_tol2 = 2 * _aten_identity_gap((Di, Hi, Wi), (Di, Ho, Wo))     # (depth in == out: weights exactly 0 and 1, the 2-D operator per plane)
    print("%s, 2-D entry (form %d): %.3g (%.3g), identity %.3g (%.3g)" % (what, code2, e2, tol2, gap2, gap_tol2))
    assert e2 <= tol2 and tol2 <= 1e-5 * max(1.0, Wo / 100.0) * max(1.0, r2.abs().max().item()), what
    assert gap2 <= gap_tol2, what
    return code, code2


ADJOINT_FORMS = [
    ("row groups, 10 row lanes", (2, 6, 24), (8, 24, 96), ROWS),
    ("row groups, rows not a multiple of 8, two column passes", (2, 11, 300), (5, 44, 1200), ROWS),
    ("row groups refused on LDS: voxel kernel, windows", (2, 6, 400), (4, 24, 1600), VOXEL_WINDOW),
    ("factor 8: voxel kernel, loop", (2, 4, 24), (4, 32, 192), VOXEL_LOOP),
    ("row groups, down-sampling", (3, 21, 40), (2, 9, 17), ROWS),
]


@pytest.mark.parametrize("row", ADJOINT_FORMS, ids=[r[0] for r in ADJOINT_FORMS])
def test_adjoint_forms(dev, row):
    what, i, o, form = row
    _check_adjoints(dev, i, o, 50 + ADJOINT_FORMS.index(row) * 5, what, form)


def test_adjoint_one_wave_per_input(dev):
    """(1, 2) -> (64, 128): the 2-D entry gathers a footprint of 64 outputs or more with one wave per input element."""
    ops = _ops()
    B, C, hw_in, hw_out = 2, 3, (1, 2), (64, 128)
    code, detail, why = bwd_plan(B_BIL, B, C, hw_in, 0, hw_out, 0)
    assert code == WAVE, (code, why)
    x, g = _rand((B, C) + hw_in, 81, 2.0), _rand((B, C) + hw_out, 82)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        xr = x.to(dtype).requires_grad_(True)
        refs[dtype], = torch.autograd.grad(F.interpolate(xr, size=list(hw_out), mode="bilinear", align_corners=True), xr, g.to(dtype))
    r = refs[torch.float64]
    tol = _tol(refs[torch.float32], r)
    got = ops.bilinear_ac_bwd(g.to(dev), hw_in)
    RAN_BWD.add(code)
    err = (got.cpu().double() - r).abs().max().item()
    gap = _gaps(x, ops.bilinear_ac(x.to(dev), hw_out).cpu(), g, got.cpu()).max().item()
    gap_tol = 2 * _aten_identity_gap((C,) + hw_in, (C,) + hw_out)
    print("one wave per input: %.3g (%.3g), identity %.3g (%.3g)" % (err, tol, gap, gap_tol))
    assert err <= tol and tol <= 1e-5 * max(1.0, hw_out[1] / 100.0) * max(1.0, r.abs().max().item())
    assert gap <= gap_tol


# ------------------------------------------------------------------------------------------------------------ ratio classes
RATIOS = [("in1", 1, 6), ("out1", 6, 1), ("same", 7, 7), ("2to5", 2, 5), ("5to13", 5, 13), ("4to16", 4, 16), ("9to3", 9, 3), ("10to4", 10, 4),
          ("65to2", 65, 2)]
REST = ((3, 5), (4, 7), (6, 10))      # (in, out) of the axes a case does not vary: depth, height, width
RATIO_CASES = [("%s-%s" % (name, axis), tuple(a if k == pos or pos == 3 else REST[k][0] for k in range(3)),
                tuple(b if k == pos or pos == 3 else REST[k][1] for k in range(3)))
               for name, a, b in RATIOS for pos, axis in enumerate(("depth", "height", "width", "all"))]


@pytest.mark.parametrize("case", RATIO_CASES, ids=[c[0] for c in RATIO_CASES])
def test_ratio_class(dev, case):
    """Every forward and adjoint entry at one sampling-ratio class on one axis (the other two up-sampled 3 -> 5, 4 -> 7, 6 -> 10) or on
    all three.  in == out on all axes must return the input bit for bit."""
    ops = _ops()
    name, i, o = case
    x = _rand((2,) + i, 90 + RATIO_CASES.index(case))
    xd = x.to(dev)
    vals = ops.disp_sample_values(o[0], 0, 1)
    RAN.add(_this(AC, 2, i, o)[0])
    y = ops.trilinear_ac(xd, o)
    _check_forward(y.cpu(), x, o, name)
    RAN.add(_this(AC_SA, 2, i, o)[0])
    yf, disp = ops.trilinear_ac_soft_argmin(xd, o, vals, 1.0)
    assert torch.equal(yf, y) and torch.equal(disp, ops.soft_argmin(y, vals, 1.0, True)), name
    _check_regression(disp, y, vals, name)
    RAN.add(_this(SA, 2, i, o)[0])
    assert (ops.trilinear_soft_argmin(xd, o, vals, 1.0) - disp).abs().max().item() <= 2e-5, name
    if i == o:
        assert torch.equal(y, xd), "%s: in == out must copy" % name
    _check_adjoints(dev, i, o, 200 + RATIO_CASES.index(case) * 5, name)
    if i == o:
        g = _rand((2,) + o, 7)
        assert torch.equal(ops.trilinear_ac_bwd(g.to(dev), i).cpu(), g), "%s: the adjoint of a copy is a copy" % name


def test_every_form_was_run(dev):
    """Last in the module: every code of both queries was launched by the tests above on this device."""
    assert RAN == REACHABLE, "forward forms not run: %s" % sorted(hex(c) for c in REACHABLE - RAN)
    assert RAN_BWD == BWD_REACHABLE, "adjoint forms not run: %s" % sorted(BWD_REACHABLE - RAN_BWD)
