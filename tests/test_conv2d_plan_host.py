"""What dmb_conv2d_f32 runs for a launch (csrc/conv2d.hip: conv2d_plan; csrc/conv3d_sk.hip: conv2d_sk_applies), seen through the query
dmb_conv2d_plan: a pure host function, so this runs without a GPU.  The estimates count workgroups over the device's compute units:
256, the MI355X's, which is also what the library assumes without a device.

Plan code = (form << 8) | index (include/dmb_hip.h): form 1 = split-K, index = (dilation 2 ? 2 : 0) + (both row tiles of a pair per
workgroup ? 1 : 0); form 2 = the tile kernel, index = the position in C2Tiles (csrc/conv2d.hip; TILES below restates the list); a
refusal is minus its DMB_E* code.

The codes of CASES were recorded from the library when the query was added.  Before that, the query was compared over 8.7 million
descriptions (every kernel size, stride, dilation and channel width on either side of what is built; widths on and off the 16-byte
rows; each alignment; both flags; 8 .. 304 compute units; every refusal) with a line-by-line transcription of the entry point it
replaces -- argument checks, the split-K gate and what the split-K launch checked before launching, the ladder of instantiations and
its tile-height estimate: no difference.  A change that moves a choice, a threshold or a refusal shows here.

GPU_CASES is the table of tests/test_conv2d_every_planned_form_gpu.py and tests/test_memory_contract_conv2d_forms_gpu.py: one launch
per reachable code at the smallest shape that reaches it -- form 2 with two or more tiles and a partial last tile along x and y of
that code's tile, form 1 with a partial 16 x 2 unit along both axes, scalar forms through W % 4 != 0."""
import pytest

from densematchingbenchmark_amd import _lib, ops

EINVAL, EUNSUPPORTED = 100001, 100002
NCU = 256
BAD, STRIDE, WINDOW = "conv2d: bad argument", "conv2d: stride must be 1 or 2", "conv2d: channel window"
TWO_GIB, GRID = "conv2d: one batch item must stay below 2 GiB", "conv2d: grid too large"
UNSUPPORTED = ("conv2d: stride 1 with kernel 1 | 3, dilation 1 | 2 (4 | 8 up to 32 output channels), output channels <= 128; "
               "stride 2 with kernel 1 | 3 (<= 64 output channels) or 5 (<= 32), dilation 1")

# index -> (32-channel row tiles, kernel, dilation, stride, 16-byte rows, output rows of a tile); every tile is 48 output columns wide
TILES = {0: (1, 3, 1, 1, False, 16), 1: (1, 3, 1, 1, True, 8), 2: (2, 3, 1, 1, False, 8), 3: (2, 3, 1, 1, True, 8), 4: (2, 3, 1, 1, True, 4),
         5: (4, 3, 1, 1, False, 4), 6: (4, 3, 1, 1, True, 2), 7: (1, 3, 2, 1, False, 16), 8: (1, 3, 2, 1, True, 16), 9: (2, 3, 2, 1, False, 8),
         10: (2, 3, 2, 1, True, 8), 11: (4, 3, 2, 1, False, 4), 12: (4, 3, 2, 1, True, 2), 13: (1, 3, 4, 1, False, 16), 14: (1, 3, 4, 1, True, 16),
         15: (1, 3, 8, 1, False, 16), 16: (1, 3, 8, 1, True, 16), 17: (1, 1, 1, 1, False, 16), 18: (1, 1, 1, 1, True, 16), 19: (2, 1, 1, 1, False, 8),
         20: (2, 1, 1, 1, True, 8), 21: (4, 1, 1, 1, False, 4), 22: (4, 1, 1, 1, True, 4), 23: (1, 3, 1, 2, False, 8), 24: (1, 3, 1, 2, True, 8),
         25: (2, 3, 1, 2, False, 4), 26: (2, 3, 1, 2, True, 4), 27: (1, 1, 1, 2, False, 8), 28: (1, 1, 1, 2, True, 8), 29: (2, 1, 1, 2, False, 4),
         30: (2, 1, 1, 2, True, 4), 31: (1, 5, 1, 2, False, 8), 32: (1, 5, 1, 2, True, 8)}
TX = 48
SPLIT_K = {0x100, 0x101, 0x102, 0x103}
# what the release library builds (0x221 .. 0x223, four rows per wave at 32 and 128 output channels: the development build only)
REACHABLE = SPLIT_K | {0x200 + k for k in TILES}
FOUR_ROWS_64 = 0x203


def scalar_of(code):
    """The code of the same layer on rows that are not 16-byte aligned."""
    key = TILES[code & 0xff]
    return 0x200 + next(k for k, t in TILES.items() if t[:4] == key[:4] and not t[4])


def _d(B, Ci, Co, H, W, k=3, s=1, dl=1, tot=None, al=(16, 16, 16), sc=0):
    """A description: channel totals default to (Ci, Co, 0 = no residual)."""
    return (B, Ci, Co, H, W, k, s, dl) + (tot or (Ci, Co, 0)) + al + (sc,)


# (what the row is there for, the description (see _d), recorded plan code, recorded message of a refusal)
CASES = [
    # ---- every instantiation of the tile kernel, on 16-byte rows and off them (Ci 24: split-K needs whole 16-channel groups)
    ("3x3 32 two rows", _d(2, 24, 32, 9, 52), 0x201, ""),
    ("3x3 32 scalar", _d(2, 24, 32, 17, 50), 0x200, ""),
    ("3x3 64 two rows: strict win", _d(2, 24, 64, 5, 52), 0x204, ""),
    ("3x3 64 four rows: tie", _d(2, 64, 64, 513, 52), 0x203, ""),
    ("3x3 64 scalar", _d(2, 24, 64, 9, 50), 0x202, ""),
    ("3x3 128 two rows", _d(2, 24, 128, 3, 52), 0x206, ""),
    ("3x3 128 scalar", _d(2, 24, 128, 5, 50), 0x205, ""),
    ("3x3 dil 2 32", _d(2, 24, 32, 17, 52, dl=2), 0x208, ""),
    ("3x3 dil 2 32 scalar", _d(2, 24, 32, 17, 50, dl=2), 0x207, ""),
    ("3x3 dil 2 64", _d(2, 24, 64, 9, 52, dl=2), 0x20a, ""),
    ("3x3 dil 2 64 scalar", _d(2, 24, 64, 9, 50, dl=2), 0x209, ""),
    ("3x3 dil 2 128 two rows", _d(2, 24, 128, 3, 52, dl=2), 0x20c, ""),
    ("3x3 dil 2 128 scalar", _d(2, 24, 128, 5, 50, dl=2), 0x20b, ""),
    ("3x3 dil 4", _d(2, 32, 32, 17, 52, dl=4), 0x20e, ""),
    ("3x3 dil 4 scalar", _d(2, 32, 32, 17, 50, dl=4), 0x20d, ""),
    ("3x3 dil 8", _d(2, 32, 32, 17, 52, dl=8), 0x210, ""),
    ("3x3 dil 8 scalar", _d(2, 32, 32, 17, 50, dl=8), 0x20f, ""),
    ("1x1 32", _d(2, 32, 32, 17, 52, k=1), 0x212, ""),
    ("1x1 32 scalar", _d(2, 32, 32, 17, 50, k=1), 0x211, ""),
    ("1x1 64", _d(2, 32, 64, 9, 52, k=1), 0x214, ""),
    ("1x1 64 scalar", _d(2, 32, 64, 9, 50, k=1), 0x213, ""),
    ("1x1 128", _d(2, 32, 128, 5, 52, k=1), 0x216, ""),
    ("1x1 128 scalar", _d(2, 32, 128, 5, 50, k=1), 0x215, ""),
    ("1x1 ignores the dilation at stride 1", _d(2, 32, 64, 9, 52, k=1, dl=2), 0x214, ""),
    ("3x3 stride 2 32", _d(2, 32, 32, 17, 104, s=2), 0x218, ""),
    ("3x3 stride 2 32 scalar", _d(2, 32, 32, 17, 101, s=2), 0x217, ""),
    ("3x3 stride 2 32: Wo % 4", _d(2, 32, 32, 17, 100, s=2), 0x217, ""),
    ("3x3 stride 2 64", _d(2, 32, 64, 9, 104, s=2), 0x21a, ""),
    ("3x3 stride 2 64 scalar", _d(2, 32, 64, 9, 101, s=2), 0x219, ""),
    ("1x1 stride 2 32", _d(2, 32, 32, 17, 104, k=1, s=2), 0x21c, ""),
    ("1x1 stride 2 32 scalar", _d(2, 32, 32, 17, 101, k=1, s=2), 0x21b, ""),
    ("1x1 stride 2 64", _d(2, 32, 64, 9, 104, k=1, s=2), 0x21e, ""),
    ("1x1 stride 2 64 scalar", _d(2, 32, 64, 9, 101, k=1, s=2), 0x21d, ""),
    ("5x5 stride 2", _d(2, 3, 32, 17, 104, k=5, s=2), 0x220, ""),
    ("5x5 stride 2 scalar", _d(2, 3, 32, 17, 101, k=5, s=2), 0x21f, ""),
    ("Co 1 .. 31 take the 32-channel tiles", _d(2, 20, 1, 9, 52), 0x201, ""),
    ("Co 33 .. 64 the 64-channel ones", _d(2, 20, 33, 5, 52), 0x204, ""),
    ("Co 97 .. 128 the 128-channel ones", _d(2, 20, 97, 3, 52), 0x206, ""),
    ("each alignment decides alone: x", _d(2, 24, 64, 9, 52, al=(8, 16, 16)), 0x202, ""),
    ("each alignment decides alone: y", _d(2, 24, 64, 9, 52, al=(16, 4, 16)), 0x202, ""),
    ("each alignment decides alone: residual", _d(2, 24, 64, 9, 52, tot=(24, 64, 64), al=(16, 16, 8)), 0x202, ""),
    ("without residual its alignment takes no part", _d(2, 24, 64, 9, 52, al=(16, 16, 4)), 0x204, ""),
    # ---- the tile height: rounds of the 512 workgroup slots x rows per wave.  [2, 64, 513, 52]: 260 tiles of 8 rows = 1 round x 4
    # against 516 tiles of 4 rows = 2 rounds x 2: a tie, which 64 channels give to four rows and 32 / 128 channels to two
    ("height: 64 channels, tie", _d(2, 64, 64, 513, 52), 0x203, ""),
    ("height: 64 channels, one row fewer: 512 tiles of 4 rows win", _d(2, 64, 64, 512, 52), 0x204, ""),
    ("height: 64 channels, the backbone's 8 x 136 x 240", _d(8, 64, 64, 136, 240), 0x204, ""),
    ("height: 32 channels at the 64-channel tie", _d(2, 64, 32, 1025, 52), 0x201, ""),
    ("height: 128 channels at the 64-channel tie", _d(2, 64, 128, 257, 52), 0x206, ""),
    ("height: 128 channels dil 2", _d(2, 64, 128, 257, 52, dl=2), 0x20c, ""),
    ("height: one batch item of the tie", _d(1, 64, 64, 513, 52, sc=1), 0x204, ""),
    # ---- split-K and its gate: at most 5 x 256 units of (16 x 2 pixels) x (32 channels)
    ("split-K 32 -> 32", _d(1, 32, 32, 64, 128), 0x100, ""),
    ("split-K 64 -> 64: both row tiles", _d(1, 64, 64, 64, 128), 0x101, ""),
    ("split-K 80 -> 64: one row tile above 64 input channels", _d(1, 80, 64, 64, 128), 0x100, ""),
    ("split-K 128 -> 128: one row tile", _d(1, 128, 128, 16, 128), 0x100, ""),
    ("split-K 64 -> 128: both row tiles of each pair", _d(1, 64, 128, 16, 128), 0x101, ""),
    ("split-K 32 -> 96: three row tiles, one each", _d(1, 32, 96, 16, 128), 0x100, ""),
    ("split-K dil 2", _d(1, 128, 128, 16, 32, dl=2), 0x102, ""),
    ("split-K dil 2 both row tiles", _d(1, 64, 64, 16, 32, dl=2), 0x103, ""),
    ("split-K 1280 units", _d(1, 32, 32, 160, 256), 0x100, ""),
    ("split-K 1281 units", _d(61, 32, 32, 6, 112), 0x201, ""),
    ("split-K 1280 units of two row tiles", _d(1, 32, 64, 80, 256), 0x101, ""),
    ("split-K 1284 units of two row tiles", _d(1, 32, 64, 6, 3424), 0x204, ""),
    ("split-K single chain", _d(1, 64, 64, 64, 128, sc=1), 0x204, ""),
    ("split-K Ci 24", _d(1, 24, 64, 64, 128), 0x204, ""),
    ("split-K Ci 144: nine channel pairs per wave", _d(1, 144, 64, 64, 128), 0x204, ""),
    ("split-K Co 48", _d(1, 32, 48, 64, 128), 0x204, ""),
    ("split-K W % 4", _d(1, 64, 64, 64, 126), 0x202, ""),
    ("split-K x align 8", _d(1, 64, 64, 64, 128, al=(8, 16, 16)), 0x202, ""),
    ("split-K y align 8", _d(1, 64, 64, 64, 128, al=(16, 8, 16)), 0x202, ""),
    ("split-K residual align 4", _d(1, 64, 64, 64, 128, tot=(64, 64, 64), al=(16, 16, 4)), 0x202, ""),
    ("split-K into channel windows", _d(1, 64, 64, 64, 128, tot=(320, 320, 128)), 0x101, ""),
    # (a window offset of c channels is 4 c H W bytes: off the 16-byte alignment only where W % 4 != 0 already rules the form out)
    ("split-K x window 8 bytes off", _d(1, 64, 64, 64, 126, tot=(65, 64, 0), al=(8, 16, 16)), 0x202, ""),
    ("split-K dil 4", _d(1, 32, 32, 16, 32, dl=4), 0x20e, ""),
    ("split-K 1x1", _d(1, 32, 32, 16, 32, k=1), 0x212, ""),
    ("split-K stride 2", _d(1, 32, 32, 16, 32, s=2), 0x218, ""),
    # ---- refusals
    ("B = 0", _d(0, 32, 32, 16, 32), -EINVAL, BAD),
    ("Ci = 0", _d(1, 0, 32, 16, 32), -EINVAL, BAD),
    ("Co = 0", _d(1, 32, 0, 16, 32), -EINVAL, BAD),
    ("H = 0", _d(1, 32, 32, 0, 32), -EINVAL, BAD),
    ("W < 0", _d(1, 32, 32, 16, -4), -EINVAL, BAD),
    ("stride 3", _d(1, 32, 32, 16, 32, s=3), -EUNSUPPORTED, STRIDE),
    ("stride 0", _d(1, 32, 32, 16, 32, s=0), -EUNSUPPORTED, STRIDE),
    ("input window", _d(1, 32, 32, 16, 32, tot=(31, 32, 0)), -EINVAL, WINDOW),
    ("output window", _d(1, 32, 32, 16, 32, tot=(32, 31, 0)), -EINVAL, WINDOW),
    ("residual window", _d(1, 32, 32, 16, 32, tot=(32, 32, 31)), -EINVAL, WINDOW),
    ("2 GiB: input item", _d(1, 32, 32, 1024, 1024, tot=(512, 32, 0)), -EUNSUPPORTED, TWO_GIB),
    ("2 GiB: output item", _d(1, 32, 32, 1024, 1024, tot=(32, 512, 0)), -EUNSUPPORTED, TWO_GIB),
    ("2 GiB: residual item", _d(1, 32, 32, 1024, 1024, tot=(32, 32, 512)), -EUNSUPPORTED, TWO_GIB),
    ("2 GiB: Ci + 8 channels", _d(1, 504, 32, 1024, 1024, tot=(511, 32, 0)), -EUNSUPPORTED, TWO_GIB),
    ("just below 2 GiB", _d(1, 503, 32, 1024, 1024, tot=(511, 511, 511)), 0x201, ""),
    ("Co 129", _d(1, 32, 129, 16, 32), -EUNSUPPORTED, UNSUPPORTED),
    ("5x5 stride 1", _d(1, 32, 32, 16, 32, k=5), -EUNSUPPORTED, UNSUPPORTED),
    ("5x5 stride 2 64", _d(1, 32, 64, 16, 32, k=5, s=2), -EUNSUPPORTED, UNSUPPORTED),
    ("kernel 2", _d(1, 32, 32, 16, 32, k=2), -EUNSUPPORTED, UNSUPPORTED),
    ("3x3 dil 3", _d(1, 32, 32, 16, 32, dl=3), -EUNSUPPORTED, UNSUPPORTED),
    ("3x3 dil 4 64", _d(1, 64, 64, 16, 32, dl=4), -EUNSUPPORTED, UNSUPPORTED),
    ("3x3 stride 2 128", _d(1, 64, 128, 16, 32, s=2), -EUNSUPPORTED, UNSUPPORTED),
    ("3x3 stride 2 dil 2", _d(1, 64, 64, 16, 32, s=2, dl=2), -EUNSUPPORTED, UNSUPPORTED),
    ("1x1 stride 2 dil 2", _d(1, 64, 64, 16, 32, k=1, s=2, dl=2), -EUNSUPPORTED, UNSUPPORTED),
    ("grid too large", _d(1 << 30, 32, 128, 4, 4), -EUNSUPPORTED, GRID),
    ("grid just fits", _d((1 << 30) - 1, 32, 128, 4, 4), 0x206, ""),
]

# (id, Ci, Co, kernel, stride, dilation, (B, H, W), plan code at 256 compute units, plan code of ONE batch item under the single-chain
#  flag).  The workloads' channel counts where split-K leaves them to the tiles; Ci 24 (no whole 16-channel groups) where it would not;
#  an odd Ci (a zero-padded last channel chunk) and output channels short of the row tile here and there.
GPU_CASES = [
    ("k3_32_scalar", 24, 32, 3, 1, 1, (2, 17, 50), 0x200, 0x200),
    ("k3_32_two", 24, 32, 3, 1, 1, (2, 9, 52), 0x201, 0x201),
    ("k3_64_scalar", 5, 64, 3, 1, 1, (2, 9, 50), 0x202, 0x202),
    ("k3_64_four", 24, 64, 3, 1, 1, (2, 513, 52), 0x203, 0x204),
    ("k3_64_two", 24, 64, 3, 1, 1, (2, 5, 52), 0x204, 0x204),
    ("k3_128_scalar", 24, 128, 3, 1, 1, (2, 5, 50), 0x205, 0x205),
    ("k3_128_two", 24, 100, 3, 1, 1, (2, 3, 52), 0x206, 0x206),
    ("k3d2_32_scalar", 24, 32, 3, 1, 2, (2, 17, 50), 0x207, 0x207),
    ("k3d2_32", 24, 32, 3, 1, 2, (2, 17, 52), 0x208, 0x208),
    ("k3d2_64_scalar", 24, 64, 3, 1, 2, (2, 9, 50), 0x209, 0x209),
    ("k3d2_64", 24, 64, 3, 1, 2, (2, 9, 52), 0x20a, 0x20a),
    ("k3d2_128_scalar", 33, 128, 3, 1, 2, (2, 5, 50), 0x20b, 0x20b),
    ("k3d2_128_two", 24, 128, 3, 1, 2, (2, 3, 52), 0x20c, 0x20c),
    ("k3d4_scalar", 32, 32, 3, 1, 4, (2, 17, 50), 0x20d, 0x20d),
    ("k3d4", 32, 32, 3, 1, 4, (2, 17, 52), 0x20e, 0x20e),
    ("k3d8_scalar", 32, 32, 3, 1, 8, (2, 17, 50), 0x20f, 0x20f),
    ("k3d8", 32, 20, 3, 1, 8, (2, 17, 52), 0x210, 0x210),
    ("k1_32_scalar", 33, 32, 1, 1, 1, (2, 17, 50), 0x211, 0x211),
    ("k1_32", 32, 32, 1, 1, 1, (2, 17, 52), 0x212, 0x212),
    ("k1_64_scalar", 32, 64, 1, 1, 1, (2, 9, 50), 0x213, 0x213),
    ("k1_64", 128, 64, 1, 1, 1, (2, 9, 52), 0x214, 0x214),
    ("k1_128_scalar", 64, 128, 1, 1, 1, (2, 5, 50), 0x215, 0x215),
    ("k1_128", 320, 128, 1, 1, 1, (2, 5, 52), 0x216, 0x216),
    ("k3s2_32_scalar", 3, 32, 3, 2, 1, (2, 17, 101), 0x217, 0x217),
    ("k3s2_32", 32, 32, 3, 2, 1, (2, 17, 104), 0x218, 0x218),
    ("k3s2_64_scalar", 32, 64, 3, 2, 1, (2, 9, 101), 0x219, 0x219),
    ("k3s2_64", 32, 64, 3, 2, 1, (2, 9, 104), 0x21a, 0x21a),
    ("k1s2_32_scalar", 32, 32, 1, 2, 1, (2, 17, 101), 0x21b, 0x21b),
    ("k1s2_32", 32, 32, 1, 2, 1, (2, 17, 104), 0x21c, 0x21c),
    ("k1s2_64_scalar", 32, 64, 1, 2, 1, (2, 9, 101), 0x21d, 0x21d),
    ("k1s2_64", 32, 48, 1, 2, 1, (2, 9, 104), 0x21e, 0x21e),
    ("k5s2_scalar", 3, 32, 5, 2, 1, (2, 17, 101), 0x21f, 0x21f),
    ("k5s2", 3, 32, 5, 2, 1, (2, 17, 104), 0x220, 0x220),
    ("sk_one", 32, 32, 3, 1, 1, (2, 5, 20), 0x100, 0x201),
    ("sk_both", 64, 64, 3, 1, 1, (2, 5, 20), 0x101, 0x204),
    ("sk_d2_one", 128, 128, 3, 1, 2, (2, 5, 20), 0x102, 0x20c),
    ("sk_d2_both", 32, 128, 3, 1, 2, (2, 5, 20), 0x103, 0x20c),
]


def _plan(desc, ncu=NCU):
    return _lib.load().dmb_conv2d_plan(*desc, ncu)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_is_the_recorded_one(case):
    lib = _lib.load()
    _, desc, code, msg = case
    assert _plan(desc) == code
    assert lib.dmb_last_error().decode() == msg
    # without a device the library counts 256 compute units on its own
    assert _plan(desc, 0) == code


def test_recorded_cases_cover_every_instantiation_and_refusal():
    codes = {c[2] for c in CASES}
    assert codes - {-EINVAL, -EUNSUPPORTED} == REACHABLE
    assert {(c[2], c[3]) for c in CASES if c[2] < 0} == {(-EINVAL, BAD), (-EUNSUPPORTED, STRIDE), (-EINVAL, WINDOW), (-EUNSUPPORTED, TWO_GIB),
                                                          (-EUNSUPPORTED, UNSUPPORTED), (-EUNSUPPORTED, GRID)}
    assert sorted(TILES) == list(range(33))


def test_four_rows_per_wave_are_planned_for_64_channels_only():
    """cost2 = 2 ceil(t2 / slots) <= 4 ceil(t4 / slots) = cost4 whatever the launch (t2 <= 2 t4), and 32 / 128 output channels give a tie
    to two rows: B in {1, 2, 3, 4, 8}, H 1 .. 599, W 4 .. 1296 in steps of 4 on 512 slots never name anything but the two-row tiles
    there -- the release library does not build the four-row ones -- while 64 channels take four rows on ties, first at [4, 64, 513, 4]."""
    lib = _lib.load()
    four = []
    for B in (1, 2, 3, 4, 8):
        for H in range(1, 600):
            for W in range(4, 1297, 4):
                d = (H, W, 3, 1, 1, 24)
                assert lib.dmb_conv2d_plan(B, 24, 32, *d, 32, 0, 16, 16, 16, 1, NCU) == 0x201
                assert lib.dmb_conv2d_plan(B, 24, 128, *d, 128, 0, 16, 16, 16, 1, NCU) == 0x206
                c64 = lib.dmb_conv2d_plan(B, 24, 64, *d, 64, 0, 16, 16, 16, 1, NCU)
                assert c64 in (FOUR_ROWS_64, 0x204)
                if c64 == FOUR_ROWS_64:
                    four.append((B * H * W, B, H, W))
            assert lib.dmb_conv2d_plan(B, 24, 128, H, 1296, 3, 1, 2, 24, 128, 0, 16, 16, 16, 1, NCU) == 0x20c
    assert len(four) == 411312 and min(four) == (4 * 513 * 4, 4, 513, 4)


def test_sweep_names_built_instantiations_only():
    """Every kernel size, stride and dilation the entry point knows, each channel width, widths on and off the 16-byte rows, small and
    large launches, forced compute-unit counts, aligned and 4-byte aligned operands, with and without the single-chain flag: no code
    outside what the release library builds; split-K never under the flag, never off the 16-byte rows, never beyond its units; and
    the tile follows the layer: the code's key is the launch's."""
    seen = set()
    for (k, s, dl) in ((3, 1, 1), (3, 1, 2), (3, 1, 4), (3, 1, 8), (1, 1, 1), (3, 2, 1), (1, 2, 1), (5, 2, 1)):
        for Co in (32, 64, 128):
            for Ci in (24, 32, 64, 128):
                for (B, H) in ((1, 1), (1, 16), (2, 33), (4, 136), (2, 513)):
                    for W in (4, 16, 20, 50, 52, 100, 104, 240):
                        for al in (16, 4):
                            for sc in (0, 1):
                                for ncu in (8, NCU):
                                    code = _lib.load().dmb_conv2d_plan(B, Ci, Co, H, W, k, s, dl, Ci, Co, Co, al, al, al, sc, ncu)
                                    if code < 0:
                                        assert code == -EUNSUPPORTED and (Co > 32 and (dl > 2 or k == 5) or Co > 64 and s == 2)
                                        continue
                                    assert code in REACHABLE, (k, s, dl, Co, Ci, B, H, W, al, sc, ncu, hex(code))
                                    v16 = W % 4 == 0 and ((W - 1) // s + 1) % 4 == 0 and al == 16
                                    if code >> 8 == ops.CONV2D_PLAN_SPLIT_K:
                                        assert not sc and v16 and (k, s) == (3, 1) and Ci % 16 == 0
                                        assert B * -(-H // 2) * -(-W // 16) * (Co // 32) <= 5 * ncu
                                        assert code & 0xff == (2 if dl == 2 else 0) + (1 if Co % 64 == 0 and Ci <= 64 else 0)
                                    else:
                                        assert TILES[code & 0xff][:5] == (Co // 32, k, dl, s, v16)
                                    seen.add(code)
    assert seen == REACHABLE


def test_ops_wrapper_takes_shapes_windows_and_the_split_k_policy(monkeypatch):
    assert ops.conv2d_plan((1, 64, 64, 128), 64, 3, ncu=NCU) == 0x101
    before = ops.split_k()
    ops.set_split_k(False)
    try:
        assert ops.conv2d_plan((1, 64, 64, 128), 64, 3, ncu=NCU) == 0x204
    finally:
        ops.set_split_k(before)
    assert ops.conv2d_plan((2, 320, 9, 52), 64, 3, dilation=2, in_window=(8, 24), ncu=NCU) == 0x20a
    assert ops.conv2d_plan((2, 32, 17, 104), 64, 5, stride=2, ncu=NCU) == -EUNSUPPORTED
    assert ops.conv2d_plan((2, 32, 17, 104), 32, 3, in_window=(0, 40), ncu=NCU) == -EINVAL

    # what reaches the library: the alignments of the WINDOW pointers, the tensors' channel totals, 0 for "no residual"
    class Fake:
        def __init__(self, ptr, shape):
            self.ptr, self.shape = ptr, shape

        def data_ptr(self):
            return self.ptr
    sent = []
    real = _lib.load()

    class Spy:
        def dmb_conv2d_plan(self, *a):
            sent.append(a)
            return real.dmb_conv2d_plan(*a)
    monkeypatch.setattr(ops._lib, "load", lambda: Spy())
    x, out, res = Fake(0x1000, (2, 9, 3, 6)), Fake(0x2000, (2, 40, 3, 6)), Fake(0x3008, (2, 35, 3, 6))
    assert ops.conv2d_plan(x, 32, 3, residual=res, in_window=(1, 8), out=out, out_ch_offset=2, res_ch_offset=3, ncu=NCU) == 0x200
    # 1 channel = 72 bytes: 8-byte aligned; 2 channels = 144 bytes: 16; 0x3008 + 216 bytes = 0x30e0: 16 although the base is not
    assert sent[-1] == (2, 8, 32, 3, 6, 3, 1, 1, 9, 40, 35, 8, 16, 16, 0, NCU)
    assert ops.conv2d_plan(x, 32, 3, in_window=(1, 8), ncu=NCU) == 0x200
    assert sent[-1] == (2, 8, 32, 3, 6, 3, 1, 1, 9, 32, 0, 8, 16, 16, 0, NCU)


@pytest.mark.parametrize("case", GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_gpu_case_reaches_its_code_with_partial_tiles_on_both_axes(case):
    """What the GPU tests rely on, so that a shape cannot go stale: the recorded code at 256 compute units, with a residual and without;
    the recorded code of one batch item under the single-chain flag; B = 2 and at most 1e5 input pixels; for form 2 at least two tiles
    and a partial last one along x and y of THAT tile, 16-byte rows exactly where the tile is a vector one, and a second code only
    where the list has another height; for form 1 a partial 16 x 2 unit along both axes."""
    name, Ci, Co, k, s, dl, (B, H, W), code, alone = case
    for rct in (0, Co):
        assert _plan((B, Ci, Co, H, W, k, s, dl, Ci, Co, rct, 16, 16, 16, 0)) == code
    assert _plan((1, Ci, Co, H, W, k, s, dl, Ci, Co, Co, 16, 16, 16, 1)) == alone
    assert B == 2 and B * H * W <= 1e5
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    if code in SPLIT_K:
        assert W % 16 and H % 2 and W > 16 and H > 2 and alone >> 8 == ops.CONV2D_PLAN_TILES
        return
    ntt, kk, dil, ss, v16, ty = TILES[code & 0xff]
    assert (ntt, kk, dil, ss) == (-(-Co // 32), k, dl, s) and v16 == (W % 4 == 0 and Wo % 4 == 0)
    assert Wo > TX and Wo % TX and Ho > ty and Ho % ty
    assert alone == code or (code, alone) == (FOUR_ROWS_64, 0x204)


def test_gpu_cases_cover_every_code():
    assert {c[7] for c in GPU_CASES} == REACHABLE
    assert len(GPU_CASES) == len(REACHABLE)
