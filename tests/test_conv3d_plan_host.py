"""What dmb_conv3d_k3_f32 runs for a launch (csrc/conv3d.hip: conv3d_plan; csrc/conv3d_s1s2.hip: conv3d_s1_plan / conv3d_s2_plan;
csrc/conv3d_sk.hip: conv3d_sk_applies), seen through the query dmb_conv3d_k3_plan: a pure host function, so this runs without a
GPU.  The estimates count workgroups over the device's compute units: 256, the MI355X's, which is also what the library assumes
without a device.

Plan code = (form << 8) | index (include/dmb_hip.h): form 1 = split-K (variant, + 4 at stride 2); 2 = stride 1 on 16-byte rows
(0 .. 3 = S1Tiles32: 48 x 4, 24 x 8, 32 x 4, 32 x 2; 4 .. 8 = S1Tiles64: 64-voxel runs, 40 x 4, 24 x 4, 32 x 4, 16 x 2); 3 = stride 1
flattened (TX 60 / 52 for 32, then for 64 output channels); 4 = stride 1 with 128 output channels; 5 = stride 2 (0 .. 3 = one / two /
four rows of 30 columns, 22 columns x 4; 4 = four rows with the dword epilogue; 5 .. 7 = dword staging for 64 / 32 / 128 output
channels); a refusal is minus its DMB_E* code.

The codes of CASES were recorded from the library when the query was added, next to a build of the commit before it whose device
code is the same instruction for instruction; tests/test_conv3d_tile_choice_host.py (unchanged) pins the stride-1 picks from before.
A change that moves a choice, a threshold or a refusal shows here.

GPU_CASES is the table of tests/test_conv3d_every_planned_form_gpu.py and tests/test_memory_contract_conv_tiles_gpu.py: one launch
per tile code at the smallest shape that reaches the code with two or more tiles and a partial last tile along every axis."""
import pytest

from densematchingbenchmark_amd import _lib, ops

EINVAL, EUNSUPPORTED = 100001, 100002
NCU = 256
UNSUPPORTED = "conv3d: output channels must be 32 or 64 (or 1: dmb_conv3d_k3_c1_f32), stride 1 or 2"
TWO_GIB = "conv3d: 8 channels of one batch item must stay below 2 GiB (32-bit buffer offsets)"

# (what the row is there for, B, Ci, Co, D, H, W, stride, alignment of x / y / residual, single-chain flag, recorded plan code,
#  recorded message of a refusal)
CASES = [
    # ---- split-K and its gate: at most 384 chains of (16 x 2 voxels) x (32 channels); 32 -> 64 at stride 2 up to 1024
    ("split-K s1 64->64", 1, 64, 64, 4, 16, 32, 1, 16, 16, 16, 0, 0x101, ""),
    ("split-K s1 single chain", 1, 64, 64, 4, 16, 32, 1, 16, 16, 16, 1, 0x208, ""),
    ("split-K s1 384 chains", 1, 32, 32, 6, 128, 16, 1, 16, 16, 16, 0, 0x101, ""),
    ("split-K s1 390 chains", 1, 32, 32, 6, 130, 16, 1, 16, 16, 16, 0, 0x203, ""),
    ("split-K s1 Co 64 384 chains", 1, 32, 64, 3, 128, 16, 1, 16, 16, 16, 0, 0x101, ""),
    ("split-K s1 Co 64 388 chains", 1, 32, 64, 3, 130, 16, 1, 16, 16, 16, 0, 0x208, ""),
    ("split-K s2 64->64", 1, 64, 64, 8, 32, 64, 2, 16, 16, 16, 0, 0x105, ""),
    ("split-K s2 single chain", 1, 64, 64, 8, 32, 64, 2, 16, 16, 16, 1, 0x500, ""),
    ("split-K s2 32->64 both row tiles, 1024 chains", 1, 32, 64, 16, 64, 128, 2, 16, 16, 16, 0, 0x107, ""),
    ("split-K s2 32->64 1040 chains", 1, 32, 64, 16, 66, 128, 2, 16, 16, 16, 0, 0x501, ""),
    ("split-K s2 64->64 beyond 384 chains", 1, 64, 64, 16, 64, 128, 2, 16, 16, 16, 0, 0x501, ""),
    ("split-K s2 32->32 small", 1, 32, 32, 8, 32, 64, 2, 16, 16, 16, 0, 0x105, ""),
    ("split-K Ci 24", 1, 24, 32, 4, 16, 32, 1, 16, 16, 16, 0, 0x203, ""),
    ("split-K Ci 80", 1, 80, 32, 4, 16, 32, 1, 16, 16, 16, 0, 0x203, ""),
    ("split-K Ci 48 both row tiles declined", 1, 48, 64, 16, 64, 128, 2, 16, 16, 16, 0, 0x501, ""),
    ("split-K W % 4", 1, 64, 64, 4, 16, 30, 1, 16, 16, 16, 0, 0x303, ""),
    ("split-K x align 8", 1, 64, 64, 4, 16, 32, 1, 8, 16, 16, 0, 0x303, ""),
    ("split-K y align 8", 1, 64, 64, 4, 16, 32, 1, 16, 8, 16, 0, 0x303, ""),
    ("split-K res align 4", 1, 64, 64, 4, 16, 32, 1, 16, 16, 4, 0, 0x303, ""),
    ("split-K s2 y align 4, Wo % 4 == 2", 1, 64, 64, 8, 32, 12, 2, 16, 4, 16, 0, 0x105, ""),
    ("split-K s2 y align 4, Wo % 4 == 0", 1, 64, 64, 8, 32, 16, 2, 16, 4, 16, 0, 0x503, ""),
    ("split-K Co 128", 1, 64, 128, 4, 16, 32, 1, 16, 16, 16, 0, 0x400, ""),
    # ---- stride 1, 32 output channels
    ("s1 32 headline", 4, 32, 32, 48, 136, 240, 1, 16, 16, 16, 0, 0x200, ""),
    ("s1 32 pick 1", 1, 32, 32, 16, 68, 168, 1, 16, 16, 16, 0, 0x201, ""),
    ("s1 32 pick 2", 2, 32, 32, 24, 68, 160, 1, 16, 16, 16, 0, 0x202, ""),
    ("s1 32 pick 2 -> 3 at one round", 1, 32, 32, 16, 64, 128, 1, 16, 16, 16, 0, 0x203, ""),
    ("s1 32 pick 3", 1, 32, 32, 12, 36, 96, 1, 16, 16, 16, 0, 0x203, ""),
    ("s1 32 KITTI", 4, 32, 32, 48, 96, 312, 1, 16, 16, 16, 0, 0x202, ""),
    ("s1 64 -> 32", 4, 64, 32, 48, 136, 240, 1, 16, 16, 16, 0, 0x200, ""),
    ("s1 32 W % 4: TX 60", 2, 32, 32, 8, 20, 118, 1, 16, 16, 16, 0, 0x300, ""),
    ("s1 32 W % 4: TX 52", 2, 32, 32, 8, 20, 102, 1, 16, 16, 16, 0, 0x301, ""),
    ("s1 32 x align 4", 2, 32, 32, 8, 20, 120, 1, 4, 16, 16, 0, 0x300, ""),
    ("s1 32 y align 8", 2, 32, 32, 8, 20, 120, 1, 16, 8, 16, 0, 0x300, ""),
    ("s1 32 res align 4: TX 52", 2, 32, 32, 8, 20, 104, 1, 16, 16, 4, 0, 0x301, ""),
    ("s1 32 output item 2 GiB", 1, 32, 32, 64, 512, 1024, 1, 16, 16, 16, 0, 0x301, ""),
    # ---- stride 1, 64 and 128 output channels
    ("s1 64 runs (quarter resolution)", 4, 64, 64, 12, 34, 60, 1, 16, 16, 16, 0, 0x204, ""),
    ("s1 64 runs need W <= 64", 4, 64, 64, 12, 34, 68, 1, 16, 16, 16, 0, 0x208, ""),
    ("s1 64 runs need W >= 32", 4, 64, 64, 12, 68, 28, 1, 16, 16, 16, 0, 0x208, ""),
    ("s1 64 40 x 4", 4, 64, 64, 24, 20, 120, 1, 16, 16, 16, 0, 0x205, ""),
    ("s1 64 24 x 4", 2, 64, 64, 3, 51, 68, 1, 16, 16, 16, 0, 0x206, ""),
    ("s1 64 32 x 4", 2, 64, 64, 3, 65, 84, 1, 16, 16, 16, 0, 0x207, ""),
    ("s1 64 16 x 2", 1, 64, 64, 8, 32, 64, 1, 16, 16, 16, 1, 0x208, ""),
    ("s1 32 -> 64", 4, 32, 64, 24, 68, 120, 1, 16, 16, 16, 0, 0x206, ""),
    ("s1 64 W % 4: TX 60", 2, 64, 64, 8, 20, 118, 1, 16, 16, 16, 0, 0x302, ""),
    ("s1 64 W % 4: TX 52", 2, 64, 64, 8, 20, 102, 1, 16, 16, 16, 0, 0x303, ""),
    ("s1 64 y align 4", 2, 64, 64, 8, 20, 120, 1, 16, 4, 16, 0, 0x302, ""),
    ("s1 64 output item 2 GiB", 1, 32, 64, 32, 512, 1024, 1, 16, 16, 16, 0, 0x303, ""),
    ("s1 128", 2, 64, 128, 6, 17, 30, 1, 16, 16, 16, 0, 0x400, ""),
    ("s1 128 W % 4", 2, 64, 128, 6, 17, 31, 1, 4, 4, 4, 0, 0x400, ""),
    # ---- stride 2
    ("s2 64 one row", 4, 64, 64, 24, 68, 120, 2, 16, 16, 16, 0, 0x500, ""),
    ("s2 32 -> 64 at full size", 4, 32, 64, 48, 136, 240, 2, 16, 16, 16, 0, 0x502, ""),
    ("s2 64 two rows", 2, 64, 64, 5, 65, 64, 2, 16, 16, 16, 0, 0x501, ""),
    ("s2 64 four rows", 2, 64, 64, 5, 129, 136, 2, 16, 16, 16, 0, 0x502, ""),
    ("s2 64 22 columns", 2, 64, 64, 9, 129, 64, 2, 16, 16, 16, 0, 0x503, ""),
    ("s2 64 y align 8: pair epilogue", 2, 64, 64, 5, 129, 136, 2, 16, 8, 16, 0, 0x502, ""),
    ("s2 64 y align 4: dword epilogue", 2, 64, 64, 5, 129, 136, 2, 16, 4, 16, 0, 0x504, ""),
    ("s2 64 res align 4: dword epilogue", 2, 64, 64, 5, 129, 136, 2, 16, 16, 4, 0, 0x504, ""),
    ("s2 64 y align 4, 22 columns", 2, 64, 64, 9, 129, 64, 2, 16, 4, 16, 0, 0x503, ""),
    ("s2 64 x align 8", 2, 64, 64, 5, 129, 136, 2, 8, 16, 16, 0, 0x505, ""),
    ("s2 64 W % 4", 2, 64, 64, 5, 129, 134, 2, 16, 16, 16, 0, 0x505, ""),
    ("s2 32", 2, 32, 32, 5, 129, 136, 2, 16, 16, 16, 0, 0x506, ""),
    ("s2 32 W % 4", 2, 16, 32, 5, 129, 135, 2, 4, 4, 4, 0, 0x506, ""),
    ("s2 128", 2, 64, 128, 5, 33, 36, 2, 16, 16, 16, 0, 0x507, ""),
    # ---- refusals
    ("B = 0", 0, 32, 32, 4, 16, 32, 1, 16, 16, 16, 0, -EINVAL, "conv3d: bad argument"),
    ("Ci = 0", 1, 0, 32, 4, 16, 32, 1, 16, 16, 16, 0, -EINVAL, "conv3d: bad argument"),
    ("W = 0", 1, 32, 32, 4, 16, 0, 2, 16, 16, 16, 0, -EINVAL, "conv3d: bad argument"),
    ("2 GiB", 1, 32, 32, 64, 1024, 1024, 1, 16, 16, 16, 0, -EUNSUPPORTED, TWO_GIB),
    ("just below 2 GiB", 1, 32, 32, 64, 1024, 1020, 1, 16, 16, 16, 0, 0x300, ""),
    ("Co 48", 2, 32, 48, 8, 64, 64, 1, 16, 16, 16, 0, -EUNSUPPORTED, UNSUPPORTED),
    ("Co 48 stride 2", 2, 32, 48, 8, 64, 64, 2, 16, 16, 16, 0, -EUNSUPPORTED, UNSUPPORTED),
    ("Co 16", 2, 32, 16, 8, 64, 64, 1, 16, 16, 16, 0, -EUNSUPPORTED, UNSUPPORTED),
    ("stride 3", 2, 32, 32, 8, 64, 64, 3, 16, 16, 16, 0, -EUNSUPPORTED, UNSUPPORTED),
    ("stride 0, Co 128", 2, 32, 128, 8, 64, 64, 0, 16, 16, 16, 0, -EUNSUPPORTED, UNSUPPORTED),
    ("s1 grid too large", 1 << 30, 32, 32, 8, 4, 4, 1, 16, 16, 16, 0, -EUNSUPPORTED, "conv3d: grid too large"),
    ("s1 grid just fits", (1 << 30) - 1, 32, 32, 8, 4, 4, 1, 16, 16, 16, 0, 0x202, ""),
    ("s2 grid too large", 1 << 30, 64, 64, 8, 4, 4, 2, 16, 16, 16, 0, -EUNSUPPORTED, "conv3d: grid too large"),
    ("s2 grid fits", 1 << 29, 64, 64, 8, 4, 4, 2, 16, 16, 16, 0, 0x501, ""),
]
SPLIT_K = {0x101, 0x105, 0x107}
# what the release library builds
REACHABLE = SPLIT_K | set(range(0x200, 0x209)) | set(range(0x300, 0x304)) | {0x400} | set(range(0x500, 0x508))

# The tile behind a code that launches a full-grid kernel, in OUTPUT voxels (columns, rows, z-slices); 0x204 walks runs of 64 voxels
# of the (y, x) plane instead of boxes.
TILES = {0x200: (48, 4, 4), 0x201: (24, 8, 4), 0x202: (32, 4, 4), 0x203: (32, 2, 4),
         0x204: "runs", 0x205: (40, 4, 2), 0x206: (24, 4, 2), 0x207: (32, 4, 2), 0x208: (16, 2, 2),
         0x300: (60, 4, 4), 0x301: (52, 4, 4), 0x302: (60, 4, 2), 0x303: (52, 4, 2), 0x400: (60, 2, 2),
         0x500: (30, 1, 2), 0x501: (30, 2, 2), 0x502: (30, 4, 2), 0x503: (22, 4, 2), 0x504: (30, 4, 2),
         0x505: (30, 4, 2), 0x506: (30, 4, 4), 0x507: (30, 4, 1)}

# (id, Ci, Co, stride, (B, D, H, W), plan code at 256 compute units, plan code of ONE batch item under the single-chain flag,
#  floats the caller's out= tensor is shifted by: 1 = an output that is only 4-byte aligned, which is what reaches code 0x504)
# The workloads' channel counts, + an odd Ci (a zero-padded last channel chunk) on candidates 0 and 1 of both stride-1 lists.
GPU_CASES = [
    ("s1_32_48x4", 32, 32, 1, (2, 5, 85, 68), 0x200, 0x203, 0),
    ("s1_32_48x4_ci5", 5, 32, 1, (2, 5, 85, 68), 0x200, 0x203, 0),
    ("s1_32_24x8", 32, 32, 1, (2, 9, 85, 52), 0x201, 0x203, 0),
    ("s1_32_24x8_ci33", 33, 32, 1, (2, 9, 85, 52), 0x201, 0x203, 0),
    ("s1_32_32x4", 32, 32, 1, (2, 5, 49, 228), 0x202, 0x203, 0),
    ("s1_32_32x2", 32, 32, 1, (2, 13, 9, 36), 0x203, 0x203, 0),
    ("s1_64_runs", 64, 64, 1, (2, 3, 43, 36), 0x204, 0x208, 0),
    ("s1_64_runs_ci33", 33, 64, 1, (2, 3, 43, 36), 0x204, 0x208, 0),
    ("s1_64_40x4", 64, 64, 1, (2, 3, 73, 100), 0x205, 0x206, 0),
    ("s1_64_40x4_ci5", 5, 64, 1, (2, 3, 73, 100), 0x205, 0x206, 0),
    ("s1_64_24x4", 64, 64, 1, (2, 3, 51, 68), 0x206, 0x208, 0),
    ("s1_64_32x4", 64, 64, 1, (2, 3, 65, 84), 0x207, 0x208, 0),
    ("s1_64_16x2", 64, 64, 1, (2, 7, 13, 20), 0x208, 0x208, 0),
    ("s1_32_flat60", 32, 32, 1, (2, 5, 5, 118), 0x300, 0x300, 0),
    ("s1_32_flat52", 32, 32, 1, (2, 5, 5, 62), 0x301, 0x301, 0),
    ("s1_64_flat60", 64, 64, 1, (2, 3, 5, 118), 0x302, 0x302, 0),
    ("s1_64_flat52", 64, 64, 1, (2, 3, 5, 62), 0x303, 0x303, 0),
    ("s1_128", 64, 128, 1, (2, 3, 3, 62), 0x400, 0x400, 0),
    ("s2_64_rows1", 64, 64, 2, (2, 13, 5, 196), 0x500, 0x500, 0),
    ("s2_64_rows2", 64, 64, 2, (2, 5, 65, 64), 0x501, 0x500, 0),
    ("s2_64_rows4", 64, 64, 2, (2, 5, 129, 136), 0x502, 0x501, 0),
    ("s2_64_narrow", 64, 64, 2, (2, 9, 129, 64), 0x503, 0x501, 0),
    ("s2_32to64_rows2", 32, 64, 2, (2, 5, 113, 68), 0x501, 0x500, 0),
    ("s2_32to64_rows1", 32, 64, 2, (2, 5, 129, 68), 0x500, 0x501, 0),
    ("s2_64_rows4_dword", 64, 64, 2, (2, 5, 9, 136), 0x504, 0x504, 1),
    ("s2_64_flat", 64, 64, 2, (2, 5, 9, 66), 0x505, 0x505, 0),
    ("s2_32_flat", 32, 32, 2, (2, 9, 9, 66), 0x506, 0x506, 0),
    ("s2_128_flat", 64, 128, 2, (2, 3, 9, 66), 0x507, 0x507, 0),
]
# Codes whose one batch item, alone, may run the SAME instantiation: the smallest tile of its list and the forms the operands
# decide, not the size.  Everywhere else the item alone is another plan.
SAME_ALONE = {0x203, 0x208, 0x500, 0x300, 0x301, 0x302, 0x303, 0x400, 0x504, 0x505, 0x506, 0x507}


def _plan(B, Ci, Co, D, H, W, stride, xa=16, ya=16, ra=16, sc=0, ncu=NCU):
    return _lib.load().dmb_conv3d_k3_plan(B, Ci, Co, D, H, W, stride, xa, ya, ra, sc, ncu)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_is_the_recorded_one(case):
    lib = _lib.load()
    assert _plan(*case[1:12]) == case[12]
    assert lib.dmb_last_error().decode() == case[13]
    # without a device the library counts 256 compute units on its own
    assert lib.dmb_conv3d_k3_plan(*case[1:12], 0) == case[12]


def test_recorded_cases_cover_every_instantiation_and_refusal():
    codes = {c[12] for c in CASES}
    assert codes - {-EINVAL, -EUNSUPPORTED} == REACHABLE
    assert {(c[12], c[13]) for c in CASES if c[12] < 0} == {
        (-EINVAL, "conv3d: bad argument"), (-EUNSUPPORTED, TWO_GIB), (-EUNSUPPORTED, UNSUPPORTED), (-EUNSUPPORTED, "conv3d: grid too large")}
    assert set(TILES) == REACHABLE - SPLIT_K


def test_sweep_names_built_instantiations_only():
    """W = 4, 8, ..., 512 and widths off the 16-byte rows; B in {1, 2, 4, 8}; small and large D x H; 32, 64 and 128 output channels;
    both strides; aligned and 4-byte aligned operands; with and without the single-chain flag: no code outside what the release
    library builds, split-K never under the flag, never at 128 channels, never on 4-byte aligned input; and the forms follow the
    operands: 16-byte rows decide between forms 2 and 3, the stride between those and form 5."""
    seen = set()
    for Co in (32, 64, 128):
        for W in list(range(4, 513, 4)) + [1, 5, 13, 30, 59, 61, 103, 105, 250, 511]:
            for B in (1, 2, 4, 8):
                for (D, H) in ((1, 1), (4, 6), (12, 34), (48, 136)):
                    for stride in (1, 2):
                        for al in (16, 4):
                            for sc in (0, 1):
                                code = _plan(B, 64, Co, D, H, W, stride, al, al, al, sc)
                                assert code in REACHABLE, (Co, W, B, D, H, stride, al, sc, code)
                                form = code >> 8
                                if form == ops.CONV_PLAN_SPLIT_K:
                                    assert not sc and Co != 128 and al == 16 and W % 4 == 0
                                elif stride == 2:
                                    assert form == ops.CONV_PLAN_S2
                                    assert ((code & 0xff) < 5) == (Co == 64 and W % 4 == 0 and al == 16)
                                elif Co == 128:
                                    assert form == ops.CONV_PLAN_S1_C128
                                else:
                                    assert form == (ops.CONV_PLAN_S1_VEC if W % 4 == 0 and al == 16 else ops.CONV_PLAN_S1_FLAT)
                                    assert ((code & 0xff) >= (4 if form == ops.CONV_PLAN_S1_VEC else 2)) == (Co == 64)
                                seen.add(code)
    # 0x107 needs 32 input channels and 0x504 an aligned input with a 4-byte aligned output: the table above has them
    assert seen == REACHABLE - {0x107, 0x504}


def _count(shape, tile):
    B, D, H, W = shape
    tx, ty, tz = tile
    return B * -(-W // tx) * -(-H // ty) * -(-D // tz)


def test_plan_index_is_the_tile_of_the_statistics_launch():
    """dmb_conv3d_k3_bnstats_f32 follows the same pick: the partial sums it writes -- one pair per workgroup and channel; a caller's
    buffer with fewer slots is written out of bounds -- are the workgroups of the tile the plan names.  Heights 4 (mod 8) make the
    four candidates' counts differ (tests/test_conv3d_tile_choice_host.py), so the count names the tile."""
    lib = _lib.load()
    seen = set()
    for B in (1, 2, 4):
        for D in (4, 5, 13, 48):
            for H in (4, 12, 36, 68, 84, 132):
                for W in range(4, 321, 4):
                    code = _plan(B, 32, 32, D, H, W, 1, sc=1)
                    assert code >> 8 == ops.CONV_PLAN_S1_VEC and (code & 0xff) < 4
                    counts = [_count((B, D, H, W), TILES[0x200 + k]) for k in range(4)]
                    partials = lib.dmb_conv3d_k3_bnstats_partials(B, 32, 32, D, H, W)
                    assert partials == counts[code & 0xff], (B, D, H, W, hex(code), partials, counts)
                    if len(set(counts)) == 4:
                        seen.add(counts.index(partials))
    assert seen == {0, 1, 2, 3}
    # any Ci, and the GPU cases themselves
    for _, Ci, Co, stride, shape, code, _, _ in GPU_CASES:
        if code >> 8 == ops.CONV_PLAN_S1_VEC and Co == 32:
            assert lib.dmb_conv3d_k3_bnstats_partials(shape[0], Ci, 32, *shape[1:]) == _count(shape, TILES[code])


def test_ops_wrapper_takes_shapes_and_the_split_k_policy():
    assert ops.conv3d_k3_plan((1, 64, 4, 16, 32), 64, ncu=NCU) == 0x101
    before = ops.split_k()
    ops.set_split_k(False)
    try:
        assert ops.conv3d_k3_plan((1, 64, 4, 16, 32), 64, ncu=NCU) == 0x208
    finally:
        ops.set_split_k(before)
    assert ops.conv3d_k3_plan((2, 64, 5, 129, 136), 64, stride=(2, 2, 2), ncu=NCU) == 0x502
    assert ops.conv3d_k3_plan((2, 64, 5, 129, 136), 48, ncu=NCU) == -EUNSUPPORTED
    with pytest.raises(_lib.DmbLibraryError):
        ops.conv3d_k3_plan((2, 64, 5, 129, 136), 64, stride=(1, 2, 2))


@pytest.mark.parametrize("case", GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_gpu_case_reaches_its_tile_with_partial_tiles_on_every_axis(case):
    """What the GPU tests rely on, so that a shape cannot go stale: the recorded code at 256 compute units with and without the
    single-chain flag (no split-K), B = 2, at most 2e5 input voxels, and along x, y and z of THAT tile at least two tiles and a
    partial last one (a one-row or one-slice tile has no partial tile along that axis); for the 64-voxel runs an odd depth above 2
    and a plane that is no whole number of runs."""
    name, Ci, Co, stride, (B, D, H, W), code, alone, out_shift = case
    ya = 4 if out_shift else 16
    for sc in (0, 1):
        assert _plan(B, Ci, Co, D, H, W, stride, 16, ya, 16, sc) == code
    assert _plan(1, Ci, Co, D, H, W, stride, 16, ya, 16, 1) == alone
    assert alone != code or code in SAME_ALONE
    assert B == 2 and B * D * H * W <= 2e5
    Do, Ho, Wo = ((e - 1) // stride + 1 for e in (D, H, W))
    if TILES[code] == "runs":
        assert D % 2 == 1 and D > 2 and (H * W) % 64 != 0 and H * W > 64
        return
    for extent, t in zip((Wo, Ho, Do), TILES[code]):
        assert extent > t and (t == 1 or extent % t != 0), (name, extent, t)


def test_gpu_cases_cover_every_tile_code():
    assert {c[5] for c in GPU_CASES} == REACHABLE - SPLIT_K
    odd = {c[5] for c in GPU_CASES if c[1] % 2}
    assert odd == {0x200, 0x201, 0x204, 0x205}
