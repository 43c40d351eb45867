"""The plan of the weight gradient that strides only height and width (stride (1, 2, 2)): dmb_conv_wgrad_plan(DMB_WGRAD_S2, ...) with
``Db == Ds >= 2``, form 5 of include/dmb_hip.h (0 / 1 = the 4 x 8 tile with 16-byte / dword staging).  A pure host function: no GPU.
Conventions, ``_plan`` and the refusal texts are those of tests/test_wgrad_plan_host.py.

CASES was recorded from the library when the form was added, with all six detail fields (tiles along x, along y, segment length,
segments, slots, channel blocks), at 256 compute units.  The six training launches are three geometries: the conv role (small = dc)
of 16 -> 32, 32 -> 64, 64 -> 128 and the transposed role (small = x) of 32 -> 16, 64 -> 32, 128 -> 64 describe the same pair of
operands.  ONE_PLANE was recorded from the parent commit's library: ``Ds == Db == 1`` keeps form 2 and its detail."""
import itertools

import pytest

from densematchingbenchmark_amd import _lib
from tests import test_wgrad_plan_host as P
from tests.test_wgrad_plan_host import BIG2, EINVAL, NCU, S2, _plan, cdiv

HW_BUILT = {0x500, 0x501}
TILE = (4, 8)

# (what the row is there for, (B, Cs, Cb, Ds, Hs, Ws, Db, Hb, Wb, ksize, dilation, align), code, detail)
CASES = [
    ("training 16 <-> 32, B 1, D 9", (1, 32, 16, 9, 32, 64, 9, 64, 128, 3, 1, 16), 0x500, (8, 8, 3, 3, 192, 1)),
    ("training 32 <-> 64, B 1, D 9", (1, 64, 32, 9, 16, 32, 9, 32, 64, 3, 1, 16), 0x500, (4, 4, 2, 5, 80, 2)),
    ("training 64 <-> 128, B 1, D 9", (1, 128, 64, 9, 8, 16, 9, 16, 32, 3, 1, 16), 0x500, (2, 2, 2, 5, 20, 8)),
    ("training 16 <-> 32, B 1, D 14", (1, 32, 16, 14, 32, 64, 14, 64, 128, 3, 1, 16), 0x500, (8, 8, 4, 4, 256, 1)),
    ("training 32 <-> 64, B 1, D 14", (1, 64, 32, 14, 16, 32, 14, 32, 64, 3, 1, 16), 0x500, (4, 4, 2, 7, 112, 2)),
    ("training 64 <-> 128, B 1, D 14", (1, 128, 64, 14, 8, 16, 14, 16, 32, 3, 1, 16), 0x500, (2, 2, 2, 7, 28, 8)),
    ("training 16 <-> 32, B 4, D 9", (4, 32, 16, 9, 32, 64, 9, 64, 128, 3, 1, 16), 0x500, (8, 8, 9, 1, 256, 1)),
    ("training 32 <-> 64, B 4, D 9", (4, 64, 32, 9, 16, 32, 9, 32, 64, 3, 1, 16), 0x500, (4, 4, 5, 2, 128, 2)),
    ("training 64 <-> 128, B 4, D 9", (4, 128, 64, 9, 8, 16, 9, 16, 32, 3, 1, 16), 0x500, (2, 2, 5, 2, 32, 8)),
    ("training 16 <-> 32, B 4, D 14", (4, 32, 16, 14, 32, 64, 14, 64, 128, 3, 1, 16), 0x500, (8, 8, 14, 1, 256, 1)),
    ("training 32 <-> 64, B 4, D 14", (4, 64, 32, 14, 16, 32, 14, 32, 64, 3, 1, 16), 0x500, (4, 4, 7, 2, 128, 2)),
    ("training 64 <-> 128, B 4, D 14", (4, 128, 64, 14, 8, 16, 14, 16, 32, 3, 1, 16), 0x500, (2, 2, 7, 2, 32, 8)),
    ("min depth, partial tile, dword", (2, 32, 16, 2, 3, 5, 2, 6, 10, 3, 1, 16), 0x501, (1, 1, 1, 2, 4, 1)),
    ("odd big extents, partial channel blocks", (2, 20, 7, 5, 7, 13, 5, 13, 25, 3, 1, 16), 0x501, (2, 2, 1, 5, 40, 1)),
    ("odd Hb alone: 16-byte rows stay", (2, 32, 32, 5, 7, 12, 5, 13, 24, 3, 1, 16), 0x500, (2, 2, 1, 5, 40, 1)),
    ("odd Wb alone decides", (2, 32, 32, 5, 7, 12, 5, 14, 23, 3, 1, 16), 0x501, (2, 2, 1, 5, 40, 1)),
    ("16-byte path, depth 14", (1, 64, 32, 14, 4, 12, 14, 8, 24, 3, 1, 16), 0x500, (2, 1, 1, 14, 28, 2)),
    ("misaligned operands", (1, 64, 32, 14, 4, 12, 14, 8, 24, 3, 1, 4), 0x501, (2, 1, 1, 14, 28, 2)),
    ("8-byte aligned operands", (1, 64, 32, 14, 4, 12, 14, 8, 24, 3, 1, 8), 0x501, (2, 1, 1, 14, 28, 2)),
    ("one voxel per plane", (1, 40, 33, 3, 1, 1, 3, 1, 1, 3, 1, 16), 0x501, (1, 1, 1, 3, 3, 4)),
    ("ring: 4 + 3", (2, 128, 64, 7, 8, 32, 7, 16, 64, 3, 1, 16), 0x500, (4, 2, 4, 2, 32, 8)),
    ("several rounds: long segments", (4, 32, 32, 12, 64, 128, 12, 128, 256, 3, 1, 16), 0x500, (16, 16, 12, 1, 256, 1)),
    ("more blocks than CUs", (1, 544, 544, 3, 4, 8, 3, 8, 16, 3, 1, 16), 0x500, (1, 1, 3, 1, 1, 289)),
]

# Ds == Db == 1, recorded from the parent commit: (description, code, detail)
ONE_PLANE = [
    ((2, 32, 32, 1, 9, 13, 1, 18, 26, 3, 1, 16), 0x201, (2, 5, 1, 1, 20, 1)),
    ((2, 32, 32, 1, 9, 13, 1, 17, 25, 3, 1, 16), 0x201, (2, 5, 1, 1, 20, 1)),
    ((4, 64, 32, 1, 32, 64, 1, 64, 128, 3, 1, 16), 0x202, (8, 8, 1, 1, 128, 2)),
    ((1, 128, 64, 1, 8, 16, 1, 16, 32, 3, 1, 16), 0x200, (2, 4, 1, 1, 8, 8)),
    ((2, 128, 56, 1, 5, 28, 1, 10, 56, 3, 1, 16), 0x200, (3, 3, 1, 1, 18, 8)),
    ((2, 128, 56, 1, 5, 28, 1, 10, 56, 3, 1, 4), 0x201, (3, 3, 1, 1, 18, 8)),
    ((1, 40, 33, 1, 1, 1, 1, 1, 1, 3, 1, 16), 0x201, (1, 1, 1, 1, 1, 4)),
    ((2, 20, 7, 1, 7, 13, 1, 13, 25, 3, 1, 16), 0x201, (2, 4, 1, 1, 16, 1)),
    ((4, 128, 128, 1, 16, 32, 1, 32, 64, 3, 1, 16), 0x202, (4, 4, 1, 1, 16, 16)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_is_the_recorded_one(case):
    _, desc, code, detail = case
    assert _plan((S2,) + desc) == (code, detail)
    assert _lib.load().dmb_last_error().decode() == ""
    assert _plan((S2,) + desc, 0) == (code, detail)     # without a device the library counts 256 compute units on its own
    B, Cs, Cb, D, H, W = desc[:6]
    ntx, nty, seg, nseg, slots, blocks = detail
    assert (ntx, nty) == (cdiv(W, TILE[1]), cdiv(H, TILE[0])) and nseg == cdiv(D, seg) and blocks == cdiv(Cs, 32) * cdiv(Cb, 32)


def test_recorded_cases_cover_the_list_and_the_training_launches():
    assert {c[2] for c in CASES} == HW_BUILT
    small = {(32, 16, 32, 64), (64, 32, 16, 32), (128, 64, 8, 16)}     # (Cs, Cb, Hs, Ws) of conv role and transposed role alike
    assert {(c[1][0], c[1][3]) + c[1][1:3] + c[1][4:6] for c in CASES[:12]} == {(B, D) + s for B in (1, 4) for D in (9, 14) for s in small}
    assert any(c[1][7] % 2 for c in CASES) and any(c[1][8] % 2 for c in CASES) and any(c[1][1] % 32 and c[1][2] % 32 for c in CASES)
    assert any(c[3][3] >= 2 and c[1][3] % c[3][2] for c in CASES), "a shorter last segment"


def _sweep():
    chans = ((8, 40), (32, 16), (16, 32), (64, 32), (128, 64), (64, 128), (128, 128), (40, 100), (20, 7))
    for (Cs, Cb), B, D, H, W, oh, ow, al in itertools.product(chans, (1, 2, 4), (2, 3, 5, 9, 14), (1, 4, 7, 8, 16, 32), (1, 5, 8, 12, 16, 64),
                                                              (0, 1), (0, 1), (16, 4)):
        yield (S2, B, Cs, Cb, D, H, W, D, 2 * H - oh, 2 * W - ow, 3, 1, al)


def test_sweep():
    """Every description of the geometry plans a built code of form 5, inside the workspace the size function asks the caller for, with
    no more slots than items; the library's own count of compute units (none here: 256) plans alike."""
    lib = _lib.load()
    n, seen = 0, set()
    for desc in _sweep():
        code, (ntx, nty, seg, nseg, slots, blocks) = _plan(desc)
        assert code in HW_BUILT, (desc, code)
        seen.add(code)
        _, B, Cs, Cb, D, H, W, _, _, Wb, _, _, al = desc
        assert (code == 0x500) == (W % 4 == 0 and Wb % 4 == 0 and al >= 16), desc
        assert slots * blocks * 27 * 1024 <= lib.dmb_conv3d_wgrad_workspace_floats(Cs, Cb), desc
        assert 1 <= slots <= B * ntx * nty * nseg and nseg == cdiv(D, seg) and 1 <= seg <= D, desc
        assert _plan(desc, 0) == (code, (ntx, nty, seg, nseg, slots, blocks)), desc
        n += 1
    assert seen == HW_BUILT and n == 9 * 3 * 5 * 6 * 6 * 2 * 2 * 2


@pytest.mark.parametrize("row", ONE_PLANE, ids=["%d" % i for i in range(len(ONE_PLANE))])
def test_one_plane_plans_as_before(row):
    desc, code, detail = row
    assert _plan((S2,) + desc) == (code, detail) and code >> 8 == 2
    assert _plan((S2,) + desc) == P.parent((S2,) + desc)


def test_refusals_keep_their_codes_and_messages():
    for name, desc, code, rest in P.CASES:
        if code < 0:
            assert _plan(desc) == (code, rest), name
    # a depth that is none of Ds, 2 Ds, 2 Ds - 1; H or W off 2n / 2n - 1 with the new depth
    for big in ((5, 8, 24), (3, 8, 24), (9, 8, 24), (4, 9, 24), (4, 6, 24), (4, 8, 22), (4, 8, 25)):
        assert _plan((S2, 1, 32, 32, 4, 4, 12) + big + (3, 1, 16)) == (-EINVAL, BIG2), big
    assert _plan((S2, 1, 32, 32, 256, 128, 128, 256, 256, 256, 3, 1, 16)) == (-P.EUNSUPPORTED, P.GIB2)     # the big operand's 32 channels
    assert _plan((S2, 0, 32, 32, 4, 4, 12, 4, 8, 24, 3, 1, 16)) == (-EINVAL, P.BAD2)
    assert NCU == 256
