"""The plan of the 2-D one-output-channel weight gradient: dmb_conv_wgrad_plan(DMB_WGRAD_2D, ...) with Co == 1, ksize 3, dilation 1
and 1 .. DMB_REFINE_HEAD_MAX_C input channels, form 7 of include/dmb_hip.h (0 = tiles of 8 rows x 32 columns, one thread per input
channel and group of pixels) -- the classifier of DeepPruner's refinement head.  A pure host function: no GPU.  Conventions,
``_plan``, ``_d`` and the refusal texts are those of tests/test_wgrad_plan_host.py.

The form has no width rule and no alignment rule and runs four workgroups per compute unit: 1024 slots at 256 compute units.  A
description with more than 16 input channels, another dilation or kernel 1 plans and refuses as on the parent commit: PARENT was
read from the library at the parent commit (and is what ``test_wgrad_plan_host.parent``, its transcription, returns)."""
import itertools

import pytest

from densematchingbenchmark_amd import _lib, ops
from tests import test_wgrad_plan_host as P
from tests.test_wgrad_plan_host import D2, EUNSUPPORTED, NCU, ROWS2D, _d, _plan, cdiv

TILE = (8, 32)
MAX_C = 16
PER_CU = 4
TILES7 = "conv2d_wgrad (1 channel): too many tiles"


def _c1(B, Ci, H, W, al=16, k=3, dl=1):
    return _d(D2, B, 1, Ci, (H, W), k=k, dl=dl, al=al)


# (what the row is there for, (B, Ci, H, W, align), detail)
CASES = [
    ("one pixel", (1, 1, 1, 1, 16), (1, 1, 8, 1, 1, 1)),
    ("one row", (1, 16, 1, 22, 16), (1, 1, 8, 1, 1, 1)),
    ("odd width below a tile", (2, 5, 5, 13, 16), (1, 1, 8, 1, 2, 1)),
    ("partial tiles both ways", (2, 16, 17, 70, 16), (3, 1, 8, 3, 18, 1)),
    ("partial tiles both ways, operands 4 bytes off", (2, 16, 17, 70, 4), (3, 1, 8, 3, 18, 1)),
    ("a narrow map", (1, 9, 40, 8, 16), (1, 1, 8, 5, 5, 1)),
    ("odd sizes past a tile", (1, 16, 33, 65, 16), (3, 1, 8, 5, 15, 1)),
    ("training 16 -> 1, B 1, 128 x 256", (1, 16, 128, 256, 16), (8, 1, 8, 16, 128, 1)),
    ("training 16 -> 1, B 4, 272 x 480", (4, 16, 272, 480, 16), (15, 1, 8, 34, 1024, 1)),
]

# read from the library at the parent commit, 256 compute units: descriptions with one output channel outside the form
PARENT = [
    (_c1(2, 17, 16, 64), (0x400, (1, 1, 8, 2, 4, 1))),
    (_c1(2, 17, 17, 960), (0x400, (15, 1, 9, 2, 60, 1))),
    (_c1(2, 17, 16, 66), (-EUNSUPPORTED, ROWS2D)),
    (_c1(2, 17, 16, 64, al=4), (-EUNSUPPORTED, ROWS2D)),
    (_c1(2, 16, 16, 64, dl=2), (0x401, (1, 2, 8, 1, 4, 1))),
    (_c1(2, 16, 16, 66, dl=2), (-EUNSUPPORTED, ROWS2D)),
    (_c1(2, 16, 16, 64, k=1), (0x404, (1, 1, 8, 2, 4, 1))),
    (_c1(2, 16, 16, 64, k=1, al=8), (-EUNSUPPORTED, ROWS2D)),
    (_c1(2, 16, 16, 64, dl=3), (-EUNSUPPORTED, P.KERNEL2D)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_is_the_recorded_one(case):
    _, (B, Ci, H, W, al), detail = case
    desc = _c1(B, Ci, H, W, al)
    assert _plan(desc) == (0x700, detail)
    assert _lib.load().dmb_last_error().decode() == ""
    assert _plan(desc, 0) == (0x700, detail)     # without a device the library counts 256 compute units on its own
    ntx, nty, seg, nseg, slots, blocks = detail
    assert (ntx, nty, seg, nseg, blocks) == (cdiv(W, TILE[1]), 1, TILE[0], cdiv(H, TILE[0]), 1)
    assert slots == min(B * ntx * nseg, PER_CU * NCU)


def test_sweep():
    """Every description of the form plans 0x700, whatever the width and the alignment, inside the workspace the size function asks
    the caller for, with no more slots than items"""
    lib = _lib.load()
    n = 0
    for Ci, W, al, B, H, ncu in itertools.product((1, 5, 16), (1, 13, 66, 960), (4, 16), (1, 4), (1, 17, 272), (NCU, 8, 304)):
        desc = _c1(B, Ci, H, W, al)
        code, (ntx, nty, seg, nseg, slots, blocks) = _plan(desc, ncu)
        assert code == 0x700, (desc, code)
        assert (ntx, nty, seg, nseg, blocks) == (cdiv(W, TILE[1]), 1, TILE[0], cdiv(H, TILE[0]), 1), desc
        assert slots == min(B * ntx * nseg, PER_CU * ncu), desc
        if ncu == NCU:     # (the size function counts the device's compute units: 256 where there is none)
            assert slots * Ci * 9 <= lib.dmb_conv2d_wgrad_workspace_floats(1, Ci), desc
        n += 1
    assert n == 3 * 4 * 2 * 2 * 3 * 3
    # the bound behind it, for any number of compute units: four slots of at most 16 x 9 floats against two of 9 x 1024 per unit
    assert PER_CU * MAX_C * 9 <= 2 * 9 * 1024


@pytest.mark.parametrize("desc,want", PARENT, ids=[str(i) for i in range(len(PARENT))])
def test_descriptions_outside_the_form_plan_as_on_the_parent(desc, want):
    assert _plan(desc) == want
    assert P.parent(desc) == want


def test_refusals_come_before_the_form():
    assert _plan(_c1(0, 16, 16, 64)) == (-P.EINVAL, P.BAD2D)
    assert _plan(_c1(1, 0, 16, 64)) == (-P.EINVAL, P.BAD2D)
    assert _plan(_c1(1, 16, 0, 64)) == (-P.EINVAL, P.BAD2D)
    assert _plan(_d(D2, 1, 0, 16, (16, 64))) == (-P.EINVAL, P.BAD2D)
    assert _plan(_c1(1, 16, 4096, 4096)) == (-EUNSUPPORTED, P.GIB2D)
    assert _plan(_c1(1 << 30, 1, 16, 64)) == (-EUNSUPPORTED, TILES7)      # the items are counted in 32 bits
    # more output channels keep form 4 and its width rule
    assert _plan(_d(D2, 2, 2, 16, (16, 64))) == P.parent(_d(D2, 2, 2, 16, (16, 64))) and _plan(_d(D2, 2, 2, 16, (16, 64)))[0] == 0x400
    assert _plan(_d(D2, 2, 2, 16, (16, 66))) == (-EUNSUPPORTED, ROWS2D)
    assert MAX_C == _lib.DEFINES["DMB_REFINE_HEAD_MAX_C"]


def test_ops_wrapper_accepts_the_form():
    assert ops.WGRAD_PLAN_C1_2D == 7
    assert ops.conv_wgrad_plan(D2, (2, 16, 17, 70), (2, 1, 17, 70), 3, 1, ncu=NCU) == (0x700, (3, 1, 8, 3, 18, 1))
    assert ops.conv_wgrad_plan(D2, (2, 16, 17, 70), (2, 1, 17, 70), 3, 1, ncu=NCU)[0] >> 8 == ops.WGRAD_PLAN_C1_2D

    class Fake:     # operands 4 bytes off a 16-byte boundary
        def __init__(self, ptr, shape):
            self.ptr, self.shape = ptr, shape

        def data_ptr(self):
            return self.ptr
    assert ops.conv_wgrad_plan(D2, Fake(0x1004, (1, 9, 40, 8)), Fake(0x2004, (1, 1, 40, 8)), 3, 1, ncu=NCU) == (0x700, (1, 1, 8, 5, 5, 1))
    assert ops.conv_wgrad_plan(D2, (1, 17, 16, 66), (1, 1, 16, 66), 3, 1, ncu=NCU)[0] == -EUNSUPPORTED


def test_the_c_abi_is_unchanged():
    assert len(_lib.header_symbols()) == 115
    assert _lib.DEFINES["DMB_ABI_VERSION"] == 13 == _lib.ABI_VERSION
