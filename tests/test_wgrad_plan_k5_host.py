"""The plan of the 5x5 small-channel weight gradient: dmb_conv_wgrad_plan(DMB_WGRAD_2D, ...) with ksize 5, dilation 1 and both channel
counts in 1 .. DMB_CONV2D_K5_MAX_C, form 6 of include/dmb_hip.h (0 = tiles of 8 rows x 32 columns, one thread per (co, ci) pair).  A
pure host function: no GPU.  Conventions, ``_plan``, ``_d`` and the refusal texts are those of tests/test_wgrad_plan_host.py.

CASES was recorded from the library when the form was added, with all six detail fields (column tiles, 1 row class, a tile's 8 rows,
row tiles, slots, channel blocks), at 256 compute units: two workgroups per compute unit, 512 slots.  The form has no width rule and
no alignment rule; a description with a channel count above 16 or another dilation plans and refuses as on the parent commit."""
import itertools

import pytest

from densematchingbenchmark_amd import _lib, ops
from tests import test_wgrad_plan_host as P
from tests.test_wgrad_plan_host import D2, EUNSUPPORTED, KERNEL2D, NCU, ROWS2D, _d, _plan, cdiv

K5_BUILT = {0x600}
TILE = (8, 32)
MAX_C = 16
TILES5 = "conv2d_wgrad (kernel 5): too many tiles"


def _k5(B, Co, Ci, H, W, al=16, dl=1):
    return _d(D2, B, Co, Ci, (H, W), k=5, dl=dl, al=al)


# (what the row is there for, (B, Co, Ci, H, W, align), code, detail)
CASES = [
    ("one pixel", (1, 1, 1, 1, 1, 16), 0x600, (1, 1, 8, 1, 1, 1)),
    ("smaller than the halo", (2, 16, 3, 2, 3, 16), 0x600, (1, 1, 8, 1, 2, 1)),
    ("partial last tile on both axes", (2, 3, 5, 19, 70, 16), 0x600, (3, 1, 8, 3, 18, 1)),
    ("14 -> 14", (2, 14, 14, 16, 40, 16), 0x600, (2, 1, 8, 2, 8, 1)),
    ("14 -> 14, operands 4 bytes off", (2, 14, 14, 16, 40, 4), 0x600, (2, 1, 8, 2, 8, 1)),
    ("16 -> 16", (1, 16, 16, 24, 72, 16), 0x600, (3, 1, 8, 3, 9, 1)),
    ("more tiles than slots", (1, 1, 1, 264, 520, 16), 0x600, (17, 1, 8, 33, 512, 1)),
    ("training 14 -> 14, B 4", (4, 14, 14, 136, 240, 16), 0x600, (8, 1, 8, 17, 512, 1)),
    ("training 9 -> 9, B 1", (1, 9, 9, 272, 480, 16), 0x600, (15, 1, 8, 34, 510, 1)),
    ("training 1 -> 1, B 4", (4, 1, 1, 272, 480, 16), 0x600, (15, 1, 8, 34, 512, 1)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_is_the_recorded_one(case):
    _, (B, Co, Ci, H, W, al), code, detail = case
    desc = _k5(B, Co, Ci, H, W, al)
    assert _plan(desc) == (code, detail)
    assert _lib.load().dmb_last_error().decode() == ""
    assert _plan(desc, 0) == (code, detail)     # without a device the library counts 256 compute units on its own
    ntx, nty, seg, nseg, slots, blocks = detail
    assert (ntx, nty, seg, nseg, blocks) == (cdiv(W, TILE[1]), 1, TILE[0], cdiv(H, TILE[0]), 1)
    assert slots == min(B * ntx * nseg, 2 * NCU)


def test_recorded_cases_cover_what_the_gpu_tests_rely_on():
    assert {c[2] for c in CASES} == K5_BUILT
    tiles = {c[0]: c[1][0] * c[3][0] * c[3][3] for c in CASES}
    assert tiles["more tiles than slots"] > 2 * NCU and tiles["partial last tile on both axes"] >= 2 * 4
    assert any(c[1][3] % TILE[0] and c[1][4] % TILE[1] and c[3][0] >= 2 and c[3][3] >= 2 for c in CASES)
    assert any(c[1][5] < 16 for c in CASES)


def _sweep():
    chans = (1, 3, 9, 14, 16)
    for Co, Ci, B, H, W, al in itertools.product(chans, chans, (1, 2, 4), (1, 7, 64, 272), (1, 5, 13, 66, 480), (16, 4)):
        yield Co, Ci, B, H, W, al


def test_sweep():
    """Every description of the form plans 0x600, whatever the width and the alignment, inside the workspace the size function asks
    the caller for, with no more slots than items; the library's own count of compute units (none here: 256) plans alike."""
    lib = _lib.load()
    n = 0
    for Co, Ci, B, H, W, al in _sweep():
        desc = _k5(B, Co, Ci, H, W, al)
        code, (ntx, nty, seg, nseg, slots, blocks) = _plan(desc)
        assert code == 0x600, (desc, code)
        assert (ntx, nty, seg, nseg, blocks) == (cdiv(W, TILE[1]), 1, TILE[0], cdiv(H, TILE[0]), 1), desc
        used = slots * Co * Ci * 25
        assert used <= lib.dmb_conv2d_wgrad_workspace_floats(Co, Ci), desc
        assert 1 <= slots <= B * ntx * nseg, desc
        assert _plan(desc, 0) == (code, (ntx, nty, seg, nseg, slots, blocks)), desc
        n += 1
    assert n == 5 * 5 * 3 * 4 * 5 * 2


def test_other_kernel_5_descriptions_are_refused_as_before():
    for Co, Ci in ((17, 16), (16, 17), (17, 17), (32, 32), (1, 40)):
        assert _plan(_k5(1, Co, Ci, 16, 64)) == (-EUNSUPPORTED, KERNEL2D), (Co, Ci)
        assert _plan(_k5(1, Co, Ci, 16, 66)) == (-EUNSUPPORTED, ROWS2D), (Co, Ci)          # the width rule still comes first there
        assert _plan(_k5(1, Co, Ci, 16, 64)) == P.parent(_k5(1, Co, Ci, 16, 64))
    for dl in (2, 3, 4, 8):
        assert _plan(_k5(1, 16, 16, 16, 64, dl=dl)) == (-EUNSUPPORTED, KERNEL2D), dl
        assert _plan(_k5(1, 16, 16, 16, 66, dl=dl)) == (-EUNSUPPORTED, ROWS2D), dl
        assert _plan(_k5(1, 16, 16, 16, 64, al=4, dl=dl)) == (-EUNSUPPORTED, ROWS2D), dl
    # the argument check and the 2 GiB check come before the form
    assert _plan(_k5(0, 1, 1, 16, 64)) == (-P.EINVAL, P.BAD2D)
    assert _plan(_k5(1, 0, 1, 16, 64)) == (-P.EINVAL, P.BAD2D)
    assert _plan(_k5(1, 1, 1, 4096, 4096)) == (-EUNSUPPORTED, P.GIB2D)
    assert _plan(_k5(1 << 30, 1, 1, 16, 64)) == (-EUNSUPPORTED, TILES5)      # the items are counted in 32 bits
    # kernels 3 and 1 on small channel counts keep form 4 and its width rule
    assert _plan(_d(D2, 2, 14, 14, (16, 64))) == P.parent(_d(D2, 2, 14, 14, (16, 64))) and _plan(_d(D2, 2, 14, 14, (16, 64)))[0] == 0x400
    assert _plan(_d(D2, 2, 14, 14, (16, 66))) == (-EUNSUPPORTED, ROWS2D)
    assert MAX_C == _lib.DEFINES["DMB_CONV2D_K5_MAX_C"]


def test_ops_wrapper_accepts_the_form():
    assert ops.conv_wgrad_plan(D2, (2, 5, 19, 70), (2, 3, 19, 70), 5, 1, ncu=NCU) == (0x600, (3, 1, 8, 3, 18, 1))

    class Fake:     # operands 4 bytes off a 16-byte boundary
        def __init__(self, ptr, shape):
            self.ptr, self.shape = ptr, shape

        def data_ptr(self):
            return self.ptr
    assert ops.conv_wgrad_plan(D2, Fake(0x1004, (2, 14, 16, 40)), Fake(0x2004, (2, 14, 16, 40)), 5, 1, ncu=NCU) == (0x600, (2, 1, 8, 2, 8, 1))
    assert ops.conv_wgrad_plan(D2, (1, 17, 16, 64), (1, 16, 16, 64), 5, 1, ncu=NCU)[0] == -EUNSUPPORTED
    assert ops.WGRAD_PLAN_K5 == 6
