"""What the up-sampling and regression entry points run for a launch (csrc/upsample_plan.h), seen through the queries dmb_upsample_plan
and dmb_upsample_bwd_plan: pure host functions, so this runs without a GPU.  One choice counts the device's compute units: 256, the
MI355X's, which is also what the library assumes without a device.

Forward code = (kernel << 8) | index (include/dmb_hip.h): kernel 1 = the z-column walk of dmb_trilinear_ac_f32, index = (flat ? 8 : 0) +
log2(zsplit); 2 = its one-thread-per-row-word kernel past 65535 rows; 3 = the z-column walk with the soft-argmin, index = (flat ? 2 : 0)
+ (four columns per thread ? 1 : 0); 4 = the volume-free pixel kernel; 5 = the k8 / s4 walk, index = (regression ? 4 : 0) + threads / 64
- 1.  Adjoint code: 1 row groups, 2 voxel kernel with register windows throughout, 3 voxel kernel with the general loop somewhere, 4 one
wave per input element.  A refusal is minus its DMB_E* code.

py_plan / py_bwd_plan restate the decisions line by line (FP32 where the library computes in FP32) and are compared with the queries
over a grid: 8 .. 304 compute units, widths with every Wo % 4 and on either side of a 256-word block, Ho on both sides of 65535, batch
sizes on both sides of every threshold, every refusal.  FORMS / BWD_FORMS record the smallest arguments that reach each code on 256
compute units -- fewest output elements, then fewest input elements; tests/test_upsample_every_planned_form_gpu.py takes its list of
forms from them and finds the launches for the device it runs on with the queries."""
import ctypes
import itertools

import numpy as np
import pytest

from densematchingbenchmark_amd import _lib

EINVAL, EUNSUPPORTED = 100001, 100002
NCU = 256
MAX_D = 256
AC, AC_SA, SA, K8, K8_SA = 1, 2, 3, 4, 5            # DMB_UPSAMPLE_*
B_AC, B_AC_SA, B_BIL = 1, 2, 3                      # DMB_UPSAMPLE_BWD_*
ROWS, VOXEL_WINDOW, VOXEL_LOOP, WAVE = 1, 2, 3, 4
F32 = np.float32
SAMPLES = "disparity sample count out of range"


def cdiv(a, b):
    return -(-a // b)


def plan(entry, B, i, o, ncu=NCU):
    detail = (ctypes.c_int * 7)()
    lib = _lib.load()
    code = lib.dmb_upsample_plan(entry, B, *i, *o, ncu, detail)
    return code, tuple(detail) if code > 0 else None, lib.dmb_last_error().decode()


def bwd_plan(entry, B, planes, hw_in, Do, hw_out, ncu=NCU):
    detail = (ctypes.c_int * 6)()
    lib = _lib.load()
    code = lib.dmb_upsample_bwd_plan(entry, B, planes, *hw_in, Do, *hw_out, ncu, detail)
    return code, tuple(detail) if code > 0 else None, lib.dmb_last_error().decode()


# ------------------------------------------------------------------------------------------------------------ the transcription
def py_flat(Ho, Wo):
    return int(not (Wo & 3 or Ho * (Wo // 4) >= 0x7fffff00))


def py_plan(entry, B, i, o, ncu=NCU):
    (Di, Hi, Wi), (Do, Ho, Wo) = i, o

    def ok(kernel, index, nx, flat, zsplit, gx, gy, gz, threads):
        return (kernel << 8) | index, (nx, flat, zsplit, gx, gy, gz, threads), ""

    if entry == AC:
        if min(B, Di, Hi, Wi, Do, Ho, Wo) <= 0:
            return -EINVAL, None, "trilinear: bad argument"
        if cdiv(cdiv(Wo, 4), 256) * Do * Ho > 0x7fffffff or B > 65535:
            return -EUNSUPPORTED, None, "trilinear: grid too large"
        if Ho > 65535:
            return ok(2, 0, 4, 0, 1, cdiv(cdiv(Wo, 4), 256) * Do * Ho, B, 1, 256)
        flat = py_flat(Ho, Wo)
        nxb = (Ho * (Wo // 4) + 255) // 256 if flat else cdiv(cdiv(Wo, 4), 256)
        nblk0 = nxb * (1 if flat else Ho) * B
        zsplit, lg = 1, 0
        while nblk0 * zsplit < 2048 and zsplit * 2 <= Do and zsplit < 16:
            zsplit, lg = zsplit * 2, lg + 1
        return ok(1, (8 if flat else 0) + lg, 4, flat, zsplit, nxb * zsplit, 1 if flat else Ho, B, 256)
    if entry == AC_SA:
        if min(B, Di, Hi, Wi, Do, Ho, Wo) <= 0:
            return -EINVAL, None, "trilinear_ac_soft_argmin: bad argument"
        if Ho > 65535 or B > 65535:
            return -EUNSUPPORTED, None, "trilinear_ac_soft_argmin: grid too large"
        if Do > MAX_D:
            return -EINVAL, None, SAMPLES
        flat = py_flat(Ho, Wo)
        if B * Ho * cdiv(Wo, 4) < 4 * 64 * ncu and Ho * Wo < 0x7fffff00:
            return ok(3, 2 if flat else 0, 1, flat, 1, (Ho * Wo + 255) // 256 if flat else cdiv(Wo, 256), 1 if flat else Ho, B, 256)
        nxb = (Ho * (Wo // 4) + 255) // 256 if flat else cdiv(cdiv(Wo, 4), 256)
        return ok(3, (2 if flat else 0) + 1, 4, flat, 1, nxb, 1 if flat else Ho, B, 256)
    if entry == SA:
        if min(B, Di, Hi, Wi, Ho, Wo) <= 0:
            return -EINVAL, None, "trilinear_soft_argmin: bad argument"
        if Do <= 0 or Do > MAX_D:
            return -EINVAL, None, SAMPLES
        if Ho > 65535 or B > 65535:
            return -EUNSUPPORTED, None, "trilinear_soft_argmin: grid too large"
        return ok(4, 0, 1, 0, 1, cdiv(Wo, 256), Ho, B, 256)
    if entry in (K8, K8_SA):
        D, H, W = Di, Hi, Wi
        if min(B, D, H, W) <= 0:
            return -EINVAL, None, "deconv_k8s4_soft_argmin: bad argument"
        if 4 * H > 65535 or B > 65535:
            return -EUNSUPPORTED, None, "deconv_k8s4_soft_argmin: grid too large"
        if entry == K8_SA and 4 * D > MAX_D:
            return -EINVAL, None, SAMPLES
        nwg = cdiv(W, 256)
        wgt = cdiv(cdiv(W, nwg), 64) * 64
        return ok(5, (4 if entry == K8_SA else 0) + wgt // 64 - 1, 4, 0, 1, nwg, 4 * H, B, wgt)
    return -EINVAL, None, "upsample_plan: no such entry point"


def ac_scale(n_in, n_out):
    return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)


def gather_range(i, scale, out):
    if scale <= 0:
        return 0, (out - 1 if i == 0 else -1)
    lo = int(np.floor(F32(i - 1) / scale)) - 1
    hi = int(np.ceil(F32(i + 1) / scale)) + 1
    return max(lo, 0), min(hi, out - 1)


def py_bwd_plan(entry, B, planes, hw_in, Do, hw_out):
    (Hi, Wi), (Ho, Wo) = hw_in, hw_out
    if entry == B_AC:
        if min(B, planes, Hi, Wi, Do, Ho, Wo) <= 0:
            return -EINVAL, None, "trilinear_bwd: bad argument"
        if Ho > 65535 or planes * Hi > 65535 or B > 65535:
            return -EUNSUPPORTED, None, "trilinear_bwd: grid too large"
    elif entry == B_AC_SA:
        if min(B, planes, Hi, Wi, Ho, Wo) <= 0:
            return -EINVAL, None, "trilinear_soft_argmin_bwd: bad argument"
        if Ho > 65535 or planes * Hi > 65535 or B > 65535:
            return -EUNSUPPORTED, None, "trilinear_soft_argmin_bwd: grid too large"
        if Do <= 0 or Do > MAX_D:
            return -EINVAL, None, SAMPLES
    elif entry == B_BIL:
        if min(B, planes, Hi, Wi, Ho, Wo) <= 0:
            return -EINVAL, None, "bilinear_bwd: bad argument"
        if planes * Hi > 65535 or B > 65535 or planes > 65535:
            return -EUNSUPPORTED, None, "bilinear_bwd: grid too large"
    else:
        return -EINVAL, None, "upsample_bwd_plan: no such entry point"
    sh, sw = ac_scale(Hi, Ho), ac_scale(Wi, Wo)
    if entry == B_BIL and Hi * Wi * 64 <= Ho * Wo:
        return WAVE, (0, 0, Hi * Wi, planes, B, 64), ""
    if sh > 0 and sw > 0 and Hi >= 2 and Wi >= 2:
        win = int(np.ceil(F32(2) / sw)) + 5
        nrmax = int(np.ceil(F32(9) / sh)) + 6
        lds = nrmax * Wi * 4
        if win <= 16 and lds <= 64 * 1024 and cdiv(Hi, 8) <= 65535 and planes <= 65535:
            return ROWS, (nrmax, lds, cdiv(Hi, 8), planes, B, 256), ""
    code = VOXEL_WINDOW
    for xl in range(Wi):
        lo, hi = gather_range(xl, sw, Wo)
        if hi - lo >= 16:
            code = VOXEL_LOOP
            break
    return code, (0, 0, cdiv(Wi, 256), planes * Hi, B, 256), ""


# ------------------------------------------------------------------------------------------------------------ recorded forms
# (what the row is, entry, B, (Di, Hi, Wi), (Do, Ho, Wo), recorded code): the smallest launch that reaches the code on 256 compute units
FORMS = [
    ("unfused row zsplit 1", AC, 1, (1, 1, 1), (1, 1, 1), 0x100),
    ("unfused row zsplit 2", AC, 1, (1, 1, 1), (2, 1, 1), 0x101),
    ("unfused row zsplit 4", AC, 1, (1, 1, 1), (4, 1, 1), 0x102),
    ("unfused row zsplit 8", AC, 1, (1, 1, 1), (8, 1, 1), 0x103),
    ("unfused row zsplit 16", AC, 1, (1, 1, 1), (16, 1, 1), 0x104),
    ("unfused flat zsplit 1", AC, 1, (1, 1, 1), (1, 1, 4), 0x108),
    ("unfused flat zsplit 2", AC, 1, (1, 1, 1), (2, 1, 4), 0x109),
    ("unfused flat zsplit 4", AC, 1, (1, 1, 1), (4, 1, 4), 0x10a),
    ("unfused flat zsplit 8", AC, 1, (1, 1, 1), (8, 1, 4), 0x10b),
    ("unfused flat zsplit 16", AC, 1, (1, 1, 1), (16, 1, 4), 0x10c),
    ("unfused, rows past grid y", AC, 1, (1, 1, 1), (1, 65536, 1), 0x200),
    ("fused row, one column", AC_SA, 1, (1, 1, 1), (1, 1, 1), 0x300),
    ("fused row, four columns", AC_SA, 2, (1, 1, 1), (1, 32768, 1), 0x301),
    ("fused flat, one column", AC_SA, 1, (1, 1, 1), (1, 1, 4), 0x302),
    ("fused flat, four columns", AC_SA, 2, (1, 1, 1), (1, 32768, 4), 0x303),
    ("volume-free pixel kernel", SA, 1, (1, 1, 1), (1, 1, 1), 0x400),
    ("k8s4 64 threads", K8, 1, (1, 1, 1), (4, 4, 4), 0x500),
    ("k8s4 128 threads", K8, 1, (1, 1, 65), (4, 4, 260), 0x501),
    ("k8s4 192 threads", K8, 1, (1, 1, 129), (4, 4, 516), 0x502),
    ("k8s4 256 threads", K8, 1, (1, 1, 193), (4, 4, 772), 0x503),
    ("k8s4 + regression 64 threads", K8_SA, 1, (1, 1, 1), (4, 4, 4), 0x504),
    ("k8s4 + regression 128 threads", K8_SA, 1, (1, 1, 65), (4, 4, 260), 0x505),
    ("k8s4 + regression 192 threads", K8_SA, 1, (1, 1, 129), (4, 4, 516), 0x506),
    ("k8s4 + regression 256 threads", K8_SA, 1, (1, 1, 193), (4, 4, 772), 0x507),
]
REACHABLE = ({0x100 + f + z for f in (0, 8) for z in range(5)} | {0x200, 0x400} | {0x300 + k for k in range(4)}
             | {0x500 + k for k in range(8)})
# (what the row is, entry, B, planes, (Hi, Wi), Do, (Ho, Wo), recorded code)
BWD_FORMS = [
    ("row groups", B_AC, 1, 1, (2, 2), 1, (2, 2), ROWS),
    ("voxel kernel, windows", B_AC, 1, 1, (1, 1), 1, (1, 1), VOXEL_WINDOW),
    ("voxel kernel, loop", B_AC, 1, 1, (1, 1), 1, (1, 17), VOXEL_LOOP),
    ("one wave per input", B_BIL, 1, 1, (1, 1), 0, (1, 64), WAVE),
]
BWD_REACHABLE = {ROWS, VOXEL_WINDOW, VOXEL_LOOP, WAVE}


@pytest.mark.parametrize("row", FORMS, ids=[r[0] for r in FORMS])
def test_form_is_the_recorded_one(row):
    _, entry, B, i, o, code = row
    assert plan(entry, B, i, o)[0] == code
    assert plan(entry, B, i, o, 0)[0] == code       # without a device the library counts 256 compute units on its own
    assert _lib.load().dmb_upsample_plan(entry, B, *i, *o, NCU, None) == code     # detail is optional


@pytest.mark.parametrize("row", BWD_FORMS, ids=[r[0] for r in BWD_FORMS])
def test_adjoint_form_is_the_recorded_one(row):
    _, entry, B, planes, hw_in, Do, hw_out, code = row
    assert bwd_plan(entry, B, planes, hw_in, Do, hw_out)[0] == code
    assert _lib.load().dmb_upsample_bwd_plan(entry, B, planes, *hw_in, Do, *hw_out, 0, None) == code


def test_recorded_forms_are_every_code_and_the_smallest_launches():
    assert {r[5] for r in FORMS} == REACHABLE and len(FORMS) == len(REACHABLE) == 24
    assert {r[7] for r in BWD_FORMS} == BWD_REACHABLE and len(BWD_FORMS) == 4
    # smallest: no launch with fewer output elements (ties: fewer input elements) reaches the code.  The extents that matter are the
    # batch and the output's (and W of the k8 / s4 input), so the search walks those up to the recorded size.
    for name, entry, B, i, o, code in FORMS:
        size = B * o[0] * o[1] * o[2]
        if entry in (K8, K8_SA):
            assert all(plan(entry, 1, (1, 1, W), (4, 4, 4 * W))[0] != code for W in range(1, i[2])), name
            continue
        if code == 0x200:     # the first height that does not fit grid y
            assert o == (1, 65536, 1) and B == 1 and plan(AC, 1, i, (1, 65535, 1))[0] == 0x100
            continue
        if size > 4096:       # the two four-column rows: the threshold B * Ho * ceil(Wo / 4) >= 65536 is met with equality
            assert B * o[1] * cdiv(o[2], 4) == 4 * 64 * NCU and o[0] == 1 and o[2] in (1, 4), name
            assert plan(entry, B, i, (1, o[1] - 1, o[2]))[0] == code - 1, name
            continue
        smaller = [(b, do, ho, wo) for b in range(1, size) for do in range(1, size // b + 1) for ho in range(1, size // (b * do) + 1)
                   for wo in range(1, size // (b * do * ho) + 1) if b * do * ho * wo < size]
        assert all(plan(entry, b, (1, 1, 1), (do, ho, wo))[0] != code for b, do, ho, wo in smaller), name


# ------------------------------------------------------------------------------------------------------------ the sweeps
WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 62, 64, 1021, 1022, 1023, 1024, 1025, 1026, 1027, 1028, 1248)
HEIGHTS = (1, 2, 64, 544, 65535, 65536)
DEPTHS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 256, 257)
NCUS = (8, 64, 256, 304)


def _same(got, want, what):
    assert got == want, (what, got, want)


def test_unfused_sweep_matches_the_transcription():
    seen = set()
    for Ho, Wo, Do in itertools.product(HEIGHTS, WIDTHS, DEPTHS):
        flat = py_flat(Ho, Wo)
        base = ((Ho * (Wo // 4) + 255) // 256) if flat else cdiv(cdiv(Wo, 4), 256) * Ho
        batches = {1, 2, 65535, 65536}
        for z in (1, 2, 4, 8):      # both sides of every doubling: nblk0 * z < 2048
            t = cdiv(2048, base * z)
            batches |= {b for b in (t - 1, t, t + 1) if 1 <= b <= 65536}
        for B in sorted(batches):
            got = plan(AC, B, (3, 5, 7), (Do, Ho, Wo))
            _same(got, py_plan(AC, B, (3, 5, 7), (Do, Ho, Wo)), (B, Do, Ho, Wo))
            if got[0] > 0:
                seen.add(got[0])
                nx, fl, zs, gx, gy, gz, th = got[1]
                assert gx >= 1 and 1 <= gy <= 65535 and 1 <= gz <= 65535 and th == 256 and nx == 4
                if got[0] >> 8 == 1:     # every plane walked once: zsplit parts, none empty
                    assert zs <= Do and zs in (1, 2, 4, 8, 16) and fl == flat
    assert seen == {c for c in REACHABLE if c >> 8 in (1, 2)}
    # the flat layout's 31-bit word index: the last width that is flat at 65535 rows, and the first that is not
    assert plan(AC, 1, (1, 1, 1), (1, 65535, 131072))[0] == 0x108 and plan(AC, 1, (1, 1, 1), (1, 65535, 131076))[0] == 0x100
    _same(plan(AC, 1, (1, 1, 1), (1, 65535, 131076)), py_plan(AC, 1, (1, 1, 1), (1, 65535, 131076)), "31 bits")
    # the compute units do not enter
    assert all(plan(AC, 3, (3, 5, 7), (9, 64, 62), n) == plan(AC, 3, (3, 5, 7), (9, 64, 62)) for n in NCUS)


def test_fused_sweep_matches_the_transcription():
    seen = set()
    for ncu, Ho, Wo in itertools.product(NCUS, HEIGHTS, WIDTHS):
        t = cdiv(4 * 64 * ncu, Ho * cdiv(Wo, 4))       # the first batch size with four columns per thread
        for B in sorted({1, 65535, 65536} | {b for b in (t - 1, t, t + 1) if 1 <= b <= 65536}):
            for Do in (1, 9, 256, 257):
                got = plan(AC_SA, B, (3, 5, 7), (Do, Ho, Wo), ncu)
                _same(got, py_plan(AC_SA, B, (3, 5, 7), (Do, Ho, Wo), ncu), (ncu, B, Do, Ho, Wo))
                if got[0] > 0:
                    seen.add(got[0])
                    assert got[1][0] == (4 if B >= t else 1) and got[1][2] == 1
                _same(plan(SA, B, (3, 5, 7), (Do, Ho, Wo), ncu), py_plan(SA, B, (3, 5, 7), (Do, Ho, Wo), ncu), (B, Do, Ho, Wo))
    assert seen == {0x300, 0x301, 0x302, 0x303}
    # one column per thread indexes pixels in 31 bits: a plane of 2^31 pixels takes four columns whatever the compute units
    big = (AC_SA, 1, (1, 1, 1), (1, 65535, 32772), 1 << 23)
    assert plan(*big)[0] == 0x303 and plan(*big) == py_plan(*big)
    assert plan(AC_SA, 1, (1, 1, 1), (1, 65535, 32764), 1 << 23)[0] == 0x302


def test_k8s4_sweep_matches_the_transcription():
    seen = set()
    for entry, W, H, D, B in itertools.product((K8, K8_SA), list(range(1, 70)) + [127, 128, 129, 191, 192, 193, 255, 256, 257, 312, 511, 512,
                                                                                 513, 640, 769], (1, 2, 16383, 16384), (1, 2, 64, 65),
                                               (1, 65535, 65536)):
        got = plan(entry, B, (D, H, W), (0, 0, 0))
        _same(got, py_plan(entry, B, (D, H, W), (0, 0, 0)), (entry, B, D, H, W))
        _same(got, plan(entry, B, (D, H, W), (4 * D, 4 * H, 4 * W), 8), "Do, Ho, Wo and ncu are not read")
        if got[0] > 0:
            seen.add(got[0])
            nx, _, _, gx, gy, gz, th = got[1]
            assert gx * th >= W and (gx - 1) * th < W and th in (64, 128, 192, 256) and (gy, gz) == (4 * H, B)
    assert seen == {0x500 + k for k in range(8)}
    assert plan(K8, 1, (1, 1, 312), (0, 0, 0))[1][3:] == (2, 4, 1, 192)      # 312 columns: 2 x 192 threads, not 256 + 56


def test_adjoint_sweep_matches_the_transcription():
    seen = set()
    sizes = (1, 2, 3, 4, 5, 9, 10, 13, 16, 24, 65, 96, 300, 400)
    for Hi, Ho in ((1, 1), (1, 7), (7, 1), (2, 5), (5, 13), (4, 16), (9, 3), (65, 2), (8, 8), (64, 256), (8, 64)):
        for Wi, Wo in itertools.product(sizes, (1, 2, 3, 4, 5, 13, 16, 17, 64, 96, 128, 1200, 1600, 3200)):
            for entry in (B_AC, B_AC_SA, B_BIL):
                a = (entry, 2, 3, (Hi, Wi), 9, (Ho, Wo))
                got = bwd_plan(*a)
                _same(got, py_bwd_plan(*a), a)
                seen.add(got[0])
                if got[0] == ROWS:
                    assert got[1][1] == got[1][0] * Wi * 4 <= 65536
    assert seen == BWD_REACHABLE
    # the shapes of the GPU module's table
    assert bwd_plan(B_AC, 1, 2, (6, 24), 4, (24, 96))[0] == ROWS and bwd_plan(B_AC, 1, 2, (6, 300), 4, (24, 1200))[0] == ROWS
    assert bwd_plan(B_AC, 1, 2, (6, 400), 4, (24, 1600))[0] == VOXEL_WINDOW and bwd_plan(B_AC, 1, 2, (6, 24), 4, (48, 192))[0] == VOXEL_LOOP
    assert bwd_plan(B_BIL, 1, 2, (1, 2), 0, (64, 128))[0] == WAVE
    # LDS: 8 -> 32 rows, sh = 7 / 31, ceil(9 / sh) + 6 = 46 rows -- 356 columns fit 64 KiB, 357 do not
    assert bwd_plan(B_AC, 1, 1, (8, 356), 1, (32, 1424))[:2] == (ROWS, (46, 46 * 356 * 4, 1, 1, 1, 256))
    assert bwd_plan(B_AC, 1, 1, (8, 357), 1, (32, 1428))[0] == VOXEL_WINDOW


def test_row_group_bounds_hold_for_every_ratio():
    """What the row-group kernel relies on and cannot check: a group's gather range never exceeds nrmax rows (it would drop the rest),
    a column window never exceeds 16 (win is its bound), and every output that blends an input lies inside that input's range --
    over every (in, out) pair up to 72 -> 160, down-sampling included, in the library's FP32 arithmetic."""
    for n_in in range(2, 73):
        for n_out in list(range(2, 161)):
            s = ac_scale(n_in, n_out)
            assert s > 0
            nrmax = int(np.ceil(F32(9) / s)) + 6
            win = int(np.ceil(F32(2) / s)) + 5
            rng = [gather_range(i, s, n_out) for i in range(n_in)]
            assert all(hi - lo + 1 <= win for lo, hi in rng), (n_in, n_out)
            for y0 in range(0, n_in, 8):
                assert rng[min(y0 + 7, n_in - 1)][1] - rng[y0][0] + 1 <= nrmax, (n_in, n_out, y0)
            src = F32(s) * np.arange(n_out, dtype=F32)
            i0 = src.astype(np.int32)
            i1 = i0 + (i0 < n_in - 1)
            for o in range(n_out):
                for i in {int(i0[o]), int(i1[o])}:
                    assert rng[i][0] <= o <= rng[i][1], (n_in, n_out, o, i)


REFUSALS = [
    (AC, 0, (1, 1, 1), (1, 1, 1), -EINVAL, "trilinear: bad argument"),
    (AC, 1, (1, 1, 1), (65536, 65536, 1), -EUNSUPPORTED, "trilinear: grid too large"),
    (AC, 65536, (1, 1, 1), (1, 1, 1), -EUNSUPPORTED, "trilinear: grid too large"),
    (AC_SA, 1, (1, 0, 1), (1, 1, 1), -EINVAL, "trilinear_ac_soft_argmin: bad argument"),
    (AC_SA, 1, (1, 1, 1), (1, 65536, 1), -EUNSUPPORTED, "trilinear_ac_soft_argmin: grid too large"),
    (AC_SA, 1, (1, 1, 1), (257, 1, 1), -EINVAL, SAMPLES),
    (SA, 1, (1, 1, 1), (1, 1, 0), -EINVAL, "trilinear_soft_argmin: bad argument"),
    (SA, 1, (1, 1, 1), (0, 1, 1), -EINVAL, SAMPLES),
    (SA, 1, (1, 1, 1), (257, 1, 1), -EINVAL, SAMPLES),
    (SA, 1, (1, 1, 1), (1, 65536, 1), -EUNSUPPORTED, "trilinear_soft_argmin: grid too large"),
    (K8, 1, (1, 1, 0), (0, 0, 0), -EINVAL, "deconv_k8s4_soft_argmin: bad argument"),
    (K8, 1, (1, 16384, 1), (0, 0, 0), -EUNSUPPORTED, "deconv_k8s4_soft_argmin: grid too large"),
    (K8_SA, 1, (65, 1, 1), (0, 0, 0), -EINVAL, SAMPLES),
    (0, 1, (1, 1, 1), (1, 1, 1), -EINVAL, "upsample_plan: no such entry point"),
    (6, 1, (1, 1, 1), (1, 1, 1), -EINVAL, "upsample_plan: no such entry point"),
]


@pytest.mark.parametrize("row", REFUSALS, ids=["%d-%s" % (i, r[5]) for i, r in enumerate(REFUSALS)])
def test_refusal(row):
    entry, B, i, o, code, msg = row
    assert plan(entry, B, i, o)[::2] == (code, msg) == py_plan(entry, B, i, o)[::2]


def test_every_nonpositive_extent_is_refused():
    for entry in (AC, AC_SA, SA):
        for k in range(7):
            for bad in (0, -1):
                a = [1] * 7
                a[k] = bad
                got = plan(entry, a[0], a[1:4], a[4:7])
                assert got[0] == -EINVAL and got == py_plan(entry, a[0], a[1:4], a[4:7]), (entry, k)
    for entry in (B_AC, B_AC_SA, B_BIL):
        for k in range(7):
            a = [1] * 7
            a[k] = 0
            got = bwd_plan(entry, a[0], a[1], a[2:4], a[4], a[5:7])
            assert got == py_bwd_plan(entry, a[0], a[1], a[2:4], a[4], a[5:7]), (entry, k)
            assert got[0] == (VOXEL_WINDOW if (entry == B_BIL and k == 4) else -EINVAL), (entry, k)
    assert bwd_plan(B_AC_SA, 1, 1, (1, 1), 257, (1, 1))[::2] == (-EINVAL, SAMPLES)
    assert bwd_plan(B_AC, 1, 1, (1, 1), 257, (1, 1))[0] == VOXEL_WINDOW
    # every clause of the three grid refusals, each at the first value refused and accepted one below it:
    # (entry, B, planes, Hi, Ho) -- Ho takes no part in the 2-D entry's grid
    grid = {B_AC: "trilinear_bwd: grid too large", B_AC_SA: "trilinear_soft_argmin_bwd: grid too large", B_BIL: "bilinear_bwd: grid too large"}
    for entry, msg in grid.items():
        clauses = [(65536, 1, 1, 1), (1, 256, 256, 1), (1, 1, 65536, 1), (1, 65536, 1, 1)] + ([(1, 1, 1, 65536)] if entry != B_BIL else [])
        for B, planes, Hi, Ho in clauses:
            a = (entry, B, planes, (Hi, 1), 1, (Ho, 1))
            assert bwd_plan(*a)[::2] == (-EUNSUPPORTED, msg) == py_bwd_plan(*a)[::2], a
            below = (entry, max(B - 1, 1), planes if planes != 65536 else 65535, (Hi - 1 if Hi > 1 else 1, 1), 1, (max(Ho - 1, 1), 1))
            assert bwd_plan(*below)[0] > 0 and bwd_plan(*below) == py_bwd_plan(*below), below
    assert bwd_plan(B_BIL, 1, 1, (1, 1), 0, (65536, 1))[0] == WAVE
    assert bwd_plan(4, 1, 1, (1, 1), 1, (1, 1))[::2] == (-EINVAL, "upsample_bwd_plan: no such entry point")


def test_entry_points_refuse_what_the_plan_refuses_without_a_device():
    """The launchers plan before they touch the device: with non-NULL pointers a refused shape returns the plan's code and launches
    nothing -- 257 output planes for the fused entries among them.  The pointers are fakes, so each shape is first shown to be
    refused by the query, and the launchers are called only where no device is visible: were a refusal ever lost, the call would
    otherwise launch on address 16.  (With a device, tests/test_upsample_every_planned_form_gpu.py calls them on real tensors.)"""
    import torch
    lib, p = _lib.load(), ctypes.c_void_p(16)
    vals = (ctypes.c_float * 260)()
    # (the query's refusal, the launcher, its arguments, the code it returns)
    calls = [
        (plan(AC_SA, 1, (3, 4, 4), (257, 8, 8)), "dmb_trilinear_ac_soft_argmin_f32", (p, p, p, 1, 3, 4, 4, 257, 8, 8, 1.0, vals, None), EINVAL),
        (plan(SA, 1, (3, 4, 4), (257, 8, 8)), "dmb_trilinear_soft_argmin_f32", (p, p, 1, 3, 4, 4, 257, 8, 8, 1.0, vals, None), EINVAL),
        (plan(SA, 1, (3, 4, 4), (9, 65536, 8)), "dmb_trilinear_soft_argmin_f32", (p, p, 1, 3, 4, 4, 9, 65536, 8, 1.0, vals, None), EUNSUPPORTED),
        (plan(K8_SA, 1, (65, 2, 2), (0, 0, 0)), "dmb_deconv3d_k8s4_c1_soft_argmin_f32", (p, p, p, p, 1, 65, 2, 2, 1.0, vals, None), EINVAL),
        (plan(AC, 65536, (1, 1, 1), (1, 1, 1)), "dmb_trilinear_ac_f32", (p, p, 65536, 1, 1, 1, 1, 1, 1, None), EUNSUPPORTED),
        (bwd_plan(B_AC, 1, 256, (256, 1), 1, (1, 1)), "dmb_trilinear_ac_bwd_f32", (p, p, p, 1, 256, 256, 1, 1, 1, 1, None), EUNSUPPORTED),
        (bwd_plan(B_AC_SA, 1, 1, (1, 1), 257, (1, 1)), "dmb_trilinear_ac_soft_argmin_bwd_f32",
         (p, p, p, None, p, p, 1, 1, 1, 1, 257, 1, 1, 1.0, vals, None), EINVAL),
        (bwd_plan(B_BIL, 1, 65536, (1, 1), 0, (1, 1)), "dmb_bilinear_ac_bwd_f32", (p, p, 1, 65536, 1, 1, 1, 1, None), EUNSUPPORTED),
    ]
    for (code, _, why), name, args, want in calls:
        assert code == -want, (name, code, why)
    assert lib.dmb_trilinear_ac_f32(None, p, 1, 1, 1, 1, 1, 1, 1, None) == EINVAL      # (a NULL operand: refused whatever the shape)
    if torch.cuda.is_available():
        return
    for (_, _, why), name, args, want in calls:
        assert getattr(lib, name)(*args) == want and lib.dmb_last_error().decode() == why, name
