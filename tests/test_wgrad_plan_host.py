"""What the three weight-gradient entry points run for a launch (csrc/wgrad.hip: wgrad_plan), seen through the query
dmb_conv_wgrad_plan: a pure host function, so this runs without a GPU.  The estimates count workgroup slots over the device's compute
units: 256, the MI355X's, which is also what the library assumes without a device.

Plan code = (form << 8) | index (include/dmb_hip.h): form 1 = stride 1 (0 / 1 / 2 = 24 columns, 32 columns, 24 columns with dword
staging), form 2 = stride 2 (0 / 1 = 2 x 12 with 16-byte / dword staging, 2 / 3 = 4 x 8), form 3 = one output channel, form 4 = 2-D
(0 .. 4 = (kernel, dilation) (3, 1), (3, 2), (3, 4), (3, 8), (1, 1)); a refusal is minus its DMB_E* code.  ``detail`` = (tiles along x,
tiles along y, segment length, segments, slots = grid x, channel blocks = grid y).

CASES was recorded from the library when the query was added.  ``parent_*`` below transcribe, line by line, the three entry points
the query replaces (argument checks, tile choice, the three copies of the segment search with their constants, the grids);
test_sweep_against_the_parent compares the query with them over a few ten-thousand descriptions.  A change that moves a choice, a
threshold, a segment length, a grid or a refusal shows here.

GPU_CASES is the table of tests/test_wgrad_every_planned_form_gpu.py and tests/test_memory_contract_wgrad_forms_gpu.py: one launch per
code at the smallest shape found that reaches it with B = 2, two or more tiles, a partial last tile on every tiled axis, a channel
count off the multiples of 32 and -- forms 1, 2 and 4 -- two or more segments, the last one shorter."""
import ctypes
import itertools

import pytest

from densematchingbenchmark_amd import _lib, ops

EINVAL, EUNSUPPORTED = 100001, 100002
NCU = 256
S1, S2, D2 = 1, 2, 4          # DMB_WGRAD_S1, DMB_WGRAD_S2, DMB_WGRAD_2D
BUILT = {0x100, 0x101, 0x102, 0x200, 0x201, 0x202, 0x203, 0x300, 0x400, 0x401, 0x402, 0x403, 0x404}
S1_TX = {0x100: 24, 0x101: 32, 0x102: 24}                                   # tiles are 4 rows high
S2_TILE = {0x200: (2, 12), 0x201: (2, 12), 0x202: (4, 8), 0x203: (4, 8)}    # (rows, columns) of the small operand
C1_TILE, D2_TX = (4, 64), 64
D2_KD = {0x400: (3, 1), 0x401: (3, 2), 0x402: (3, 4), 0x403: (3, 8), 0x404: (1, 1)}
TAPS = {1: 27, 2: 27, 3: 27, 4: 9}      # per form: what a slot's partial result is sized for in the workspace

BAD1, BAD2, BAD2D = "conv3d_wgrad: bad argument", "conv3d_s2_wgrad: bad argument", "conv2d_wgrad: bad argument"
GIB1 = "conv3d_wgrad: 32 channels of one batch item must stay below 2 GiB"
GIB2 = "conv3d_s2_wgrad: 32 channels of one batch item must stay below 2 GiB"
GIB2D = "conv2d_wgrad: 32 channels of one image must stay below 2 GiB"
TILES1 = "conv3d_wgrad (1 channel): too many tiles"
BIG2 = "conv3d_s2_wgrad: the big tensor must be 2n or 2n - 1 per axis"
ROWS2D = "conv2d_wgrad: the width must be a multiple of 4 and the tensors 16-byte aligned"
KERNEL2D = "conv2d_wgrad: kernel 1, or kernel 3 with dilation 1, 2, 4 or 8 (stride 1)"
KIND = "conv_wgrad_plan: kind must be DMB_WGRAD_S1, DMB_WGRAD_S2 or DMB_WGRAD_2D"


def cdiv(a, b):
    return -(-a // b)


def _d(kind, B, Co, Ci, dims, big=None, k=3, dl=1, al=16):
    """A description in the query's argument order (without ncu and detail).  dims: (D, H, W), 2-D: (H, W); stride 2: the small
    operand's, and ``big`` the big one's (default: twice the small one's)."""
    D, H, W = (1,) + tuple(dims) if len(dims) == 2 else dims
    if kind == S2 and big is None:
        big = (2 * D, 2 * H, 2 * W)
    return (kind, B, Co, Ci, D, H, W) + tuple(big or (0, 0, 0)) + (k, dl, al)


def _plan(desc, ncu=NCU):
    """(code, detail) of the query; a refusal: (minus its code, its message)"""
    lib = _lib.load()
    detail = (ctypes.c_int * 6)(*([-1] * 6))
    code = lib.dmb_conv_wgrad_plan(*desc, ncu, detail)
    return (code, tuple(detail)) if code >= 0 else (code, lib.dmb_last_error().decode())


# ---------------------------------------------------------------------------------------------- the parent's entry points, transcribed
def _slots_per_block(Co, Ci, ncu, per_cu=1):
    return max(1, per_cu * ncu // (cdiv(Co, 32) * cdiv(Ci, 32)))


def _ws3(Co, Ci, ncu):
    return cdiv(Co, 32) * cdiv(Ci, 32) * _slots_per_block(Co, Ci, ncu) * 27 * 1024


def parent_s1(B, Ci, Co, D, H, W, align, ncu):
    """dmb_conv3d_k3_wgrad_f32 before the plan"""
    if B <= 0 or Ci <= 0 or Co <= 0 or D <= 0 or H <= 0 or W <= 0:
        return -EINVAL, BAD1
    if 32 * D * H * W * 4 >= 0x7fffffff:
        return -EUNSUPPORTED, GIB1
    if Co == 1:
        ntx, nty = cdiv(W, 64), cdiv(H, 4)
        nt = B * D * ntx * nty
        if nt > 0x7fffffff:
            return -EUNSUPPORTED, TILES1
        g = max(1, min(4 * ncu, nt, _ws3(Co, Ci, ncu) // (Ci * 27)))
        return 0x300, (ntx, nty, 1, D, g, cdiv(Ci, 32))
    nblk = cdiv(Co, 32) * cdiv(Ci, 32)
    wide = cdiv(W, 32) * 32 < cdiv(W, 24) * 24
    ntx, nty = cdiv(W, 32 if wide else 24), cdiv(H, 4)
    nslots = _slots_per_block(Co, Ci, ncu)
    zseg, best = D, 1e30
    for nz in range(1, D + 1):
        zs = cdiv(D, nz)
        if zs < 4 and nz > 1:
            break
        cost = float(cdiv(B * ntx * nty * cdiv(D, zs), nslots)) * (zs + 0.5)
        if cost < best - 1e-9:
            best, zseg = cost, zs
    nzs = cdiv(D, zseg)
    v16 = W % 4 == 0 and align >= 16
    nused = min(B * ntx * nty * nzs, nslots)
    if v16 and wide:
        return 0x101, (ntx, nty, zseg, nzs, nused, nblk)
    if v16:
        return 0x100, (ntx, nty, zseg, nzs, nused, nblk)
    return 0x102, (cdiv(W, 24), nty, zseg, nzs, nused, nblk)


def parent_s2(B, Cs, Cb, Ds, Hs, Ws, Db, Hb, Wb, align, ncu):
    """dmb_conv3d_k3s2_wgrad_f32 before the plan"""
    if B <= 0 or Cs <= 0 or Cb <= 0 or Ds <= 0 or Hs <= 0 or Ws <= 0:
        return -EINVAL, BAD2
    if Db not in (2 * Ds, 2 * Ds - 1) or Hb not in (2 * Hs, 2 * Hs - 1) or Wb not in (2 * Ws, 2 * Ws - 1):
        return -EINVAL, BIG2
    if 32 * Db * Hb * Wb * 4 >= 0x7fffffff:
        return -EUNSUPPORTED, GIB2
    v16 = Ws % 4 == 0 and Wb % 4 == 0 and align >= 16
    nblk = cdiv(Cs, 32) * cdiv(Cb, 32)
    nslots = _slots_per_block(Cs, Cb, ncu)

    def plan(TY, TX, eff):
        ntx_, nty_ = cdiv(Ws, TX), cdiv(Hs, TY)
        best, zseg_ = 1e30, Ds
        for nz in range(1, Ds + 1):
            zs = cdiv(Ds, nz)
            if zs < 4 and nz > 1:
                break
            cost = float(cdiv(B * ntx_ * nty_ * cdiv(Ds, zs), nslots)) * (zs + 1.0)
            if cost < best - 1e-9:
                best, zseg_ = cost, zs
        return best * (TY * TX) / eff, zseg_
    (cost_a, zseg_a), (cost_b, zseg_b) = plan(2, 12, 1.0), plan(4, 8, 1.1)
    wide = cost_b < cost_a
    zseg = zseg_b if wide else zseg_a
    ntx, nty = cdiv(Ws, 8 if wide else 12), cdiv(Hs, 4 if wide else 2)
    nzs = cdiv(Ds, zseg)
    nused = min(B * ntx * nty * nzs, nslots)
    return 0x200 + (2 if wide else 0) + (0 if v16 else 1), (ntx, nty, zseg, nzs, nused, nblk)


def parent_2d(B, Ci, Co, H, W, ksize, dilation, align, ncu):
    """dmb_conv2d_wgrad_f32 and launch_wgrad2d before the plan"""
    if B <= 0 or Ci <= 0 or Co <= 0 or H <= 0 or W <= 0:
        return -EINVAL, BAD2D
    if 32 * H * W * 4 >= 0x7fffffff:
        return -EUNSUPPORTED, GIB2D
    if W % 4 != 0 or align < 16:
        return -EUNSUPPORTED, ROWS2D
    if ksize == 3 and dilation in (1, 2, 4, 8):
        index, DIL = {1: 0, 2: 1, 4: 2, 8: 3}[dilation], dilation
    elif ksize == 1:
        index, DIL = 4, 1
    else:
        return -EUNSUPPORTED, KERNEL2D
    nblk, nslots = cdiv(Co, 32) * cdiv(Ci, 32), _slots_per_block(Co, Ci, ncu, 2)
    ntx, HC = cdiv(W, 64), cdiv(H, DIL)
    yseg, best = HC, 1e30
    for ny in range(1, HC + 1):
        ysz = cdiv(HC, ny)
        if ysz < 8 and ny > 1:
            break
        cost = float(cdiv(B * ntx * DIL * cdiv(HC, ysz), nslots)) * (ysz + 2.0)
        if cost < best - 1e-9:
            best, yseg = cost, ysz
    nys = cdiv(HC, yseg)
    return 0x400 + index, (ntx, DIL, yseg, nys, min(B * ntx * DIL * nys, nslots), nblk)


def parent(desc, ncu=NCU):
    kind, B, Co, Ci, D, H, W, Db, Hb, Wb, k, dl, al = desc
    if kind == S1:
        return parent_s1(B, Ci, Co, D, H, W, al, ncu)
    if kind == S2:
        return parent_s2(B, Co, Ci, D, H, W, Db, Hb, Wb, al, ncu)
    return parent_2d(B, Ci, Co, H, W, k, dl, al, ncu)


# (what the row is there for, the description (see _d), recorded code, recorded (segment length, segments, slots) or message of a refusal)
CASES = [
    # ---- stride 1: the training shapes (256 x 512 crops, B = 4: W = 128 at full resolution of the volume, 64 at half, 32 at quarter)
    ("s1 training 32 -> 32 full", _d(S1, 4, 32, 32, (48, 64, 128)), 0x101, (48, 1, 256)),
    ("s1 training 64 -> 32 first unit", _d(S1, 4, 32, 64, (48, 64, 128)), 0x101, (48, 1, 128)),
    ("s1 training 64 -> 64 half", _d(S1, 4, 64, 64, (24, 32, 64)), 0x101, (24, 1, 64)),
    ("s1 training 64 -> 64 quarter", _d(S1, 4, 64, 64, (12, 16, 32)), 0x101, (4, 3, 48)),
    ("s1 training classifier head", _d(S1, 4, 1, 32, (48, 64, 128)), 0x300, (1, 48, 1024)),
    # ---- stride 1: the width classes (32 columns where they compute fewer: W = 25 .. 32, 49 .. 64, 73 .. 96 and from 97 on)
    ("s1 W 24: one 24-column tile", _d(S1, 2, 32, 32, (9, 5, 24)), 0x100, (5, 2, 8)),
    ("s1 W 28: 32 columns", _d(S1, 2, 32, 32, (9, 5, 28)), 0x101, (5, 2, 8)),
    ("s1 W 48: two 24-column tiles", _d(S1, 2, 32, 32, (9, 5, 48)), 0x100, (5, 2, 16)),
    ("s1 W 52: 64 against 72", _d(S1, 2, 32, 32, (9, 5, 52)), 0x101, (5, 2, 16)),
    ("s1 W 68: 72 against 96", _d(S1, 2, 32, 32, (9, 5, 68)), 0x100, (5, 2, 24)),
    ("s1 W 96: a tie goes to 24 columns", _d(S1, 2, 32, 32, (9, 5, 96)), 0x100, (5, 2, 32)),
    ("s1 W 30: dword copies on the 32-column class's split", _d(S1, 2, 32, 32, (9, 5, 30)), 0x102, (5, 2, 8)),
    ("s1 W 50: dword copies", _d(S1, 2, 32, 32, (9, 5, 50)), 0x102, (5, 2, 16)),
    ("s1 misaligned operands: dword copies", _d(S1, 2, 32, 32, (9, 5, 52), al=4), 0x102, (5, 2, 16)),
    ("s1 8-byte aligned operands", _d(S1, 2, 32, 32, (9, 5, 48), al=8), 0x102, (5, 2, 16)),
    # ---- stride 1: the z split.  One round whatever the split: the shortest segments; zs < 4 stops the search
    ("s1 D 7: 4 + 3", _d(S1, 2, 32, 32, (7, 5, 52)), 0x101, (4, 2, 16)),
    ("s1 D 6: segments of 3 are not tried", _d(S1, 2, 32, 32, (6, 5, 52)), 0x101, (6, 1, 8)),
    ("s1 D 5: one segment", _d(S1, 2, 32, 32, (5, 5, 52)), 0x101, (5, 1, 8)),
    ("s1 one round: 256 items on 256 slots", _d(S1, 4, 32, 32, (16, 16, 128)), 0x101, (4, 4, 256)),
    ("s1 four segments would take a second round: three of 6 + 6 + 4", _d(S1, 5, 32, 32, (16, 16, 128)), 0x101, (6, 3, 240)),
    ("s1 slots shared by four channel blocks", _d(S1, 2, 64, 64, (9, 5, 52)), 0x101, (5, 2, 16)),
    ("s1 more blocks than CUs: one slot each", _d(S1, 1, 544, 544, (4, 4, 24)), 0x100, (4, 1, 1)),
    ("s1 Co 1 .. 31 but 1 take the tiles", _d(S1, 2, 2, 32, (9, 5, 52)), 0x101, (5, 2, 16)),
    # ---- one output channel
    ("c1 grid = tiles", _d(S1, 2, 1, 20, (2, 5, 70)), 0x300, (1, 2, 16)),
    ("c1 grid = four workgroups per CU", _d(S1, 2, 1, 32, (24, 64, 128)), 0x300, (1, 24, 1024)),
    ("c1 grid = what the workspace holds", _d(S1, 4, 1, 2048, (48, 64, 128)), 0x300, (1, 48, 128)),
    # ---- stride 2: the training shapes
    ("s2 training 32 <-> 64 full / half", _d(S2, 4, 64, 32, (24, 32, 64)), 0x202, (24, 1, 128)),
    ("s2 training 64 <-> 64 half / quarter", _d(S2, 4, 64, 64, (12, 16, 32)), 0x202, (12, 1, 64)),
    # ---- stride 2: the cost crossover at one channel block (256 slots): [2, ., 9, 13, 13] is 2 x 7 x 2 = 28 items of 2 x 12 or
    # 2 x 4 x 2 = 16 of 4 x 8 per segment, one round either way: 24 against 32 / 1.1 voxels per plane
    ("s2 one round: 2 x 12", _d(S2, 2, 32, 32, (9, 13, 13), big=(18, 26, 26)), 0x201, (5, 2, 56)),
    ("s2 16 blocks, 16 slots: 4 x 8 in one round against two", _d(S2, 2, 128, 128, (9, 13, 13), big=(18, 26, 26)), 0x203, (9, 1, 16)),
    ("s2 the issue's 1 x 9 x 13 at 128 -> 128", _d(S2, 2, 128, 128, (1, 9, 13), big=(2, 18, 26)), 0x203, (1, 1, 12)),
    ("s2 16-byte rows", _d(S2, 2, 32, 32, (9, 13, 12)), 0x200, (5, 2, 28)),
    ("s2 4 x 8 on 16-byte rows", _d(S2, 2, 128, 56, (7, 5, 28)), 0x202, (4, 2, 32)),
    ("s2 small width % 4 alone decides", _d(S2, 2, 32, 32, (9, 13, 14)), 0x201, (5, 2, 56)),
    ("s2 big width % 4 alone decides", _d(S2, 2, 32, 32, (9, 13, 12), big=(18, 26, 23)), 0x201, (5, 2, 28)),
    ("s2 misaligned operands", _d(S2, 2, 128, 56, (7, 5, 28), al=4), 0x203, (4, 2, 32)),
    ("s2 D 7: 4 + 3", _d(S2, 2, 32, 32, (7, 13, 12)), 0x200, (4, 2, 28)),
    ("s2 D 6: one segment", _d(S2, 2, 32, 32, (6, 13, 12)), 0x200, (6, 1, 14)),
    ("s2 odd big extents", _d(S2, 2, 32, 32, (5, 7, 12), big=(9, 13, 23)), 0x201, (5, 1, 8)),
    # ---- 2-D: every (kernel, dilation); the y split of a row class (segments of fewer than 8 rows are not tried)
    ("2d k3", _d(D2, 2, 32, 32, (15, 68)), 0x400, (8, 2, 8)),
    ("2d k3 dil 2", _d(D2, 2, 32, 32, (30, 68), dl=2), 0x401, (8, 2, 16)),
    ("2d k3 dil 4", _d(D2, 2, 32, 32, (60, 68), dl=4), 0x402, (8, 2, 32)),
    ("2d k3 dil 8", _d(D2, 2, 32, 32, (117, 68), dl=8), 0x403, (8, 2, 64)),
    ("2d k1", _d(D2, 2, 32, 32, (15, 68), k=1), 0x404, (8, 2, 8)),
    ("2d k1 ignores the dilation", _d(D2, 2, 32, 32, (15, 68), k=1, dl=3), 0x404, (8, 2, 8)),
    ("2d 14 rows: one segment", _d(D2, 2, 32, 32, (14, 68)), 0x400, (14, 1, 4)),
    ("2d 16 rows: 8 + 8", _d(D2, 2, 32, 32, (16, 68)), 0x400, (8, 2, 8)),
    ("2d one round: 512 items on 512 slots", _d(D2, 4, 32, 32, (256, 256)), 0x400, (8, 32, 512)),
    ("2d several rounds: longer segments", _d(D2, 4, 32, 32, (256, 320)), 0x400, (11, 24, 480)),
    ("2d AcfNet confidence head 192 -> 64", _d(D2, 4, 64, 192, (256, 512)), 0x400, (52, 5, 42)),
    # ---- refusals
    ("s1 B = 0", _d(S1, 0, 32, 32, (4, 4, 24)), -EINVAL, BAD1),
    ("s1 Ci = 0", _d(S1, 1, 32, 0, (4, 4, 24)), -EINVAL, BAD1),
    ("s1 W < 0", _d(S1, 1, 32, 32, (4, 4, -4)), -EINVAL, BAD1),
    ("s1 2 GiB", _d(S1, 1, 32, 32, (256, 256, 256)), -EUNSUPPORTED, GIB1),
    ("s1 just below 2 GiB", _d(S1, 1, 32, 32, (256, 256, 255)), 0x102, (256, 1, 256)),
    ("c1 too many tiles", _d(S1, 1 << 21, 1, 32, (64, 64, 64)), -EUNSUPPORTED, TILES1),
    ("s2 B = 0", _d(S2, 0, 32, 32, (4, 4, 12)), -EINVAL, BAD2),
    ("s2 Hs = 0", _d(S2, 1, 32, 32, (4, 0, 12)), -EINVAL, BAD2),
    ("s2 big depth", _d(S2, 1, 32, 32, (4, 4, 12), big=(9, 8, 24)), -EINVAL, BIG2),
    ("s2 big width", _d(S2, 1, 32, 32, (4, 4, 12), big=(8, 8, 22)), -EINVAL, BIG2),
    ("s2 2 GiB", _d(S2, 1, 32, 32, (128, 128, 128)), -EUNSUPPORTED, GIB2),
    ("2d Co = 0", _d(D2, 1, 0, 32, (16, 64)), -EINVAL, BAD2D),
    ("2d 2 GiB", _d(D2, 1, 32, 32, (4096, 4096)), -EUNSUPPORTED, GIB2D),
    ("2d W % 4", _d(D2, 1, 32, 32, (16, 66)), -EUNSUPPORTED, ROWS2D),
    ("2d misaligned", _d(D2, 1, 32, 32, (16, 64), al=8), -EUNSUPPORTED, ROWS2D),
    ("2d kernel 5", _d(D2, 1, 32, 32, (16, 64), k=5), -EUNSUPPORTED, KERNEL2D),
    ("2d k3 dil 3", _d(D2, 1, 32, 32, (16, 64), dl=3), -EUNSUPPORTED, KERNEL2D),
    ("kind 3 is a form, not an entry point", _d(3, 1, 32, 32, (4, 4, 24)), -EINVAL, KIND),
]

# (id, kind, Co, Ci, (B, D, H, W) of the own / small operand (2-D: (B, H, W)), kernel, dilation, plan code at 256 compute units, plan
#  code of ONE batch item).  Stride 2: Co / Ci = the small / big operand's channels, the big operand is 2n - 1 per axis where the
#  code is a dword one and 2n elsewhere.
GPU_CASES = [
    ("s1_24", S1, 24, 32, (2, 7, 5, 44), 3, 1, 0x100, 0x100),
    ("s1_32", S1, 32, 24, (2, 9, 5, 52), 3, 1, 0x101, 0x101),
    ("s1_24_dword", S1, 40, 32, (2, 7, 5, 50), 3, 1, 0x102, 0x102),
    ("s2_2x12", S2, 24, 32, (2, 7, 3, 16), 3, 1, 0x200, 0x200),
    ("s2_2x12_dword", S2, 32, 24, (2, 7, 3, 14), 3, 1, 0x201, 0x201),
    ("s2_4x8", S2, 128, 56, (2, 7, 5, 28), 3, 1, 0x202, 0x200),
    ("s2_4x8_dword", S2, 128, 56, (2, 11, 5, 13), 3, 1, 0x203, 0x201),
    ("c1", S1, 1, 20, (2, 2, 5, 70), 3, 1, 0x300, 0x300),
    ("2d_k3", D2, 24, 32, (2, 15, 68), 3, 1, 0x400, 0x400),
    ("2d_k3d2", D2, 32, 24, (2, 29, 68), 3, 2, 0x401, 0x401),
    ("2d_k3d4", D2, 40, 32, (2, 59, 68), 3, 4, 0x402, 0x402),
    ("2d_k3d8", D2, 32, 24, (2, 117, 68), 3, 8, 0x403, 0x403),
    ("2d_k1", D2, 24, 40, (2, 15, 68), 1, 1, 0x404, 0x404),
]


def gpu_case_shapes(case):
    """(shape of a, shape of b) of a GPU_CASES row, in the order ops.conv_wgrad_plan and the kernels take them: stride 1 and 2-D
    (x, dc), stride 2 (small, big)"""
    _, kind, Co, Ci, dims, _, _, code, _ = case
    B, sp = dims[0], tuple(dims[1:])
    if kind == S2:
        big = tuple(2 * v - (code & 1) for v in sp)
        return (B, Co) + sp, (B, Ci) + big
    return (B, Ci) + sp, (B, Co) + sp


def _gpu_desc(case, B=None):
    _, kind, Co, Ci, dims, k, dl, _, _ = case
    a, b = gpu_case_shapes(case)
    return _d(kind, B or dims[0], Co, Ci, dims[1:], big=b[2:] if kind == S2 else None, k=k, dl=dl)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_is_the_recorded_one(case):
    _, desc, code, rest = case
    got, detail = _plan(desc)
    assert got == code, hex(got) if got >= 0 else detail
    assert (detail[2:5] if code >= 0 else detail) == rest
    assert _lib.load().dmb_last_error().decode() == (rest if code < 0 else "")
    assert _plan(desc, 0) == (got, detail)     # without a device the library counts 256 compute units on its own
    assert desc[0] not in (S1, S2, D2) or _plan(desc) == parent(desc)
    assert _lib.load().dmb_conv_wgrad_plan(*desc, NCU, None) == code     # detail is optional


def test_recorded_cases_cover_every_instantiation_and_refusal():
    assert {c[2] for c in CASES if c[2] >= 0} == BUILT
    assert {(c[2], c[3]) for c in CASES if c[2] < 0} == {
        (-EINVAL, BAD1), (-EUNSUPPORTED, GIB1), (-EUNSUPPORTED, TILES1), (-EINVAL, BAD2), (-EINVAL, BIG2), (-EUNSUPPORTED, GIB2),
        (-EINVAL, BAD2D), (-EUNSUPPORTED, GIB2D), (-EUNSUPPORTED, ROWS2D), (-EUNSUPPORTED, KERNEL2D), (-EINVAL, KIND)}
    assert {_lib.DEFINES[k] for k in ("DMB_WGRAD_S1", "DMB_WGRAD_S2", "DMB_WGRAD_2D")} == {S1, S2, D2}


def _workspace(code, Co, Ci):
    lib = _lib.load()
    return lib.dmb_conv2d_wgrad_workspace_floats(Co, Ci) if code >> 8 == 4 else lib.dmb_conv3d_wgrad_workspace_floats(Co, Ci)


def _sweep():
    chans = ((1, 32), (1, 20), (8, 40), (32, 32), (64, 32), (32, 64), (64, 64), (128, 128), (40, 100), (544, 32))
    for (Co, Ci), B, D, H, W, al in itertools.product(chans, (1, 2, 4), (1, 4, 6, 7, 9, 12, 24, 48), (1, 5, 16, 64), (5, 24, 30, 52, 64, 96, 128), (16, 4)):
        yield _d(S1, B, Co, Ci, (D, H, W), al=al)
    for (Co, Ci), B, D, H, W, odd, al in itertools.product(chans[2:], (1, 2, 4), (1, 4, 7, 9, 12, 24), (1, 5, 13, 32), (5, 8, 12, 13, 24, 64), (0, 1), (16, 4)):
        yield _d(S2, B, Co, Ci, (D, H, W), big=(2 * D - odd, 2 * H, 2 * W - odd), al=al)
    for (Co, Ci), B, H, W, (k, dl) in itertools.product(chans[2:], (1, 2, 4), (1, 7, 14, 15, 16, 30, 59, 117, 256, 540), (4, 64, 68, 256, 960),
                                                        ((3, 1), (3, 2), (3, 4), (3, 8), (1, 1), (1, 2), (3, 3), (5, 1))):
        yield _d(D2, B, Co, Ci, (H, W), k=k, dl=dl)


def test_sweep_against_the_parent():
    """Every detail field equal to the transcription of the three entry points the plan replaces; no code outside the 13 the library
    builds; the planned grid never writes past the workspace the size functions ask the caller for."""
    n, seen = 0, set()
    for desc in _sweep():
        got = _plan(desc)
        assert got == parent(desc), desc
        n += 1
        if got[0] < 0:
            continue
        code, (ntx, nty, seg, nseg, slots, blocks) = got
        assert code in BUILT, (desc, hex(code))
        seen.add(code)
        Co, Ci = desc[2], desc[3]
        used = slots * Ci * 27 if code == 0x300 else slots * blocks * TAPS[code >> 8] * 1024
        assert used <= _workspace(code, Co, Ci), desc
        assert blocks == (cdiv(Ci, 32) if code == 0x300 else cdiv(Co, 32) * cdiv(Ci, 32)) and 1 <= slots <= desc[1] * ntx * nty * nseg
    assert seen == BUILT and 30000 <= n <= 60000


def test_ops_wrapper_takes_shapes_and_tensors(monkeypatch):
    assert ops.conv_wgrad_plan(S1, (2, 24, 9, 5, 52), (2, 32, 9, 5, 52), ncu=NCU) == (0x101, (2, 2, 5, 2, 16, 1))
    assert ops.conv_wgrad_plan(S2, (2, 128, 9, 13, 13), (2, 128, 18, 26, 26), ncu=NCU) == (0x203, (2, 4, 9, 1, 16, 16))
    assert ops.conv_wgrad_plan(D2, (2, 32, 117, 68), (2, 32, 117, 68), 3, 8, ncu=NCU) == (0x403, (2, 8, 8, 2, 64, 1))
    assert ops.conv_wgrad_plan(D2, (2, 32, 117, 66), (2, 32, 117, 66), 3, 8, ncu=NCU)[0] == -EUNSUPPORTED

    class Fake:     # what reaches the library from tensors: the two operands' alignment together
        def __init__(self, ptr, shape):
            self.ptr, self.shape = ptr, shape

        def data_ptr(self):
            return self.ptr
    assert ops.conv_wgrad_plan(S1, Fake(0x1000, (2, 32, 9, 5, 52)), Fake(0x2008, (2, 32, 9, 5, 52)), ncu=NCU)[0] == 0x102
    assert ops.conv_wgrad_plan(S1, Fake(0x1000, (2, 32, 9, 5, 52)), Fake(0x2010, (2, 32, 9, 5, 52)), ncu=NCU)[0] == 0x101


@pytest.mark.parametrize("case", GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_gpu_case_reaches_its_code_with_partial_tiles_and_a_short_last_segment(case):
    """What the GPU tests rely on, so that a shape cannot go stale: see the module's docstring."""
    name, kind, Co, Ci, dims, k, dl, code, alone = case
    a, b = gpu_case_shapes(case)
    got, (ntx, nty, seg, nseg, slots, blocks) = _plan(_gpu_desc(case))
    assert got == code and _plan(_gpu_desc(case, B=1))[0] == alone
    assert ops.conv_wgrad_plan(kind, a, b, k, dl, ncu=NCU) == (got, (ntx, nty, seg, nseg, slots, blocks))
    B, (H, W) = dims[0], dims[-2:]
    assert B == 2 and 4 * (B * a[1] * _numel(a[2:]) + B * b[1] * _numel(b[2:])) <= 5 << 20      # operands of a few MB at most
    assert Co % 32 or Ci % 32 or code == 0x300
    if code >> 8 == 4:
        assert D2_KD[code] == (k, dl) and ntx == cdiv(W, D2_TX) >= 2 and W % D2_TX and nty == dl
        extent = cdiv(H, dl)
        assert H % dl or dl == 1          # row classes of unequal length
    else:
        ty, tx = {1: (4, S1_TX.get(code)), 2: S2_TILE.get(code), 3: C1_TILE}[code >> 8]
        assert (ntx, nty) == (cdiv(W, tx), cdiv(H, ty)) and ntx * nty >= 2 and W % tx and H % ty and ntx >= 2 and nty >= 2
        extent = dims[1]
    if code == 0x300:
        assert (seg, nseg) == (1, extent) and Ci % 32
        return
    assert nseg == cdiv(extent, seg) >= 2 and extent % seg, "two or more segments, the last one shorter"
    if code in (0x102, 0x201, 0x203):     # dword forms: through the width, with aligned operands
        assert W % 4 or (kind == S2 and b[-1] % 4)
    else:
        assert W % 4 == 0 and b[-1] % 4 == 0


def _numel(shape):
    n = 1
    for v in shape:
        n *= v
    return n


def test_gpu_cases_cover_every_code():
    assert {c[7] for c in GPU_CASES} == BUILT and len(GPU_CASES) == len(BUILT)
