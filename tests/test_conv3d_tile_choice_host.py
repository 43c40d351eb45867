"""Which tile the stride-1 32 -> 32 convolution takes (csrc/conv3d_s1s2.hip: s1_pick32 over S1Tiles32), seen through the three pure
host functions that depend on it: the number of BatchNorm partial sums the caller must provide room for (= workgroups of the chosen
tile; too few is an out-of-bounds write), the fused head's workspace (= workgroups of the 48 x 4 tile x 1800 floats) and whether the
plain launch would take that tile too.  The expected values were recorded from the library BEFORE the tile tables were derived from
the S1Cfg types; a change that moves a pick shows here.  The estimate counts rounds over the device's compute units: 256, the
MI355X's, which is also what the library assumes without a device.

Candidates: 0 = 48 x 4, 1 = 24 x 8, 2 = 32 x 4, 3 = 32 x 2 (columns x rows, 4 z-slices each).  The heights are 4 (mod 8), so that
the four candidates' workgroup counts all differ and the partial count names the pick -- except the anchor and the boundary shape."""
import pytest

from densematchingbenchmark_amd import _lib

# ((B, D, H, W), partials at Ci = Co = 32, head workspace floats, head preferred)
CASES = [
    ((4, 48, 136, 240), 8160, 8160 * 1800, 1),   # the headline shape: 4 * 12 * 34 * 5 workgroups of 48 x 4
    ((4, 48, 36, 240), 2160, 3888000, 1),        # pick 0 (counts 2160 / 2400 / 3456 / 6912)
    ((1, 16, 68, 168), 252, 489600, 0),          # pick 1 (272 / 252 / 408 / 816)
    ((2, 24, 68, 160), 1020, 1468800, 0),        # pick 2 (816 / 756 / 1020 / 2040)
    ((1, 16, 84, 160), 420, 604800, 0),          # pick 2 at the fewest workgroups the estimate gives it: 420 > 256, it stays 2
    ((1, 16, 64, 128), 512, 345600, 0),          # pick 2 by estimate, exactly 256 workgroups of 32 x 4 = one per CU: -> pick 3
    ((1, 16, 68, 128), 204, 367200, 1),          # one tile row more (272 workgroups of 32 x 4): the estimate takes pick 0
    ((1, 12, 36, 96), 162, 97200, 0),            # pick 3 by estimate (54 / 60 / 81 / 162)
]


def _count(shape, tx, ty):
    B, D, H, W = shape
    return B * -(-W // tx) * -(-H // ty) * -(-D // 4)


@pytest.mark.parametrize("shape,partials,workspace,preferred", CASES)
def test_stride1_tile_choice_is_the_recorded_one(shape, partials, workspace, preferred):
    lib = _lib.load()
    B, D, H, W = shape
    got = (lib.dmb_conv3d_k3_bnstats_partials(B, 32, 32, D, H, W), lib.dmb_conv3d_k3_head_workspace_floats(B, D, H, W),
           lib.dmb_conv3d_k3_head_preferred(B, D, H, W))
    assert got == (partials, workspace, preferred)
    assert workspace == _count(shape, 48, 4) * 1800
    assert preferred == (partials == _count(shape, 48, 4))


def test_recorded_cases_cover_every_pick():
    """What the list above claims about itself: away from the anchor and the boundary shape the four counts differ, and each of
    the four candidates is the recorded pick at least once."""
    tiles = [(48, 4), (24, 8), (32, 4), (32, 2)]
    seen = set()
    for shape, partials, _, _ in CASES:
        counts = [_count(shape, tx, ty) for tx, ty in tiles]
        assert partials in counts
        if shape[2] % 8 == 4:
            assert len(set(counts)) == 4
            seen.add(counts.index(partials))
    assert seen == {0, 1, 2, 3}
    assert _count((1, 16, 64, 128), 32, 4) == 256 and _count((1, 16, 64, 128), 32, 2) == 512


def test_stride1_statistics_and_head_refusals():
    lib = _lib.load()
    assert lib.dmb_conv3d_k3_bnstats_partials(1, 32, 32, 16, 64, 126) == 0      # W % 4 != 0
    assert lib.dmb_conv3d_k3_head_workspace_floats(1, 16, 64, 126) == 0
    assert lib.dmb_conv3d_k3_head_preferred(1, 16, 64, 126) == 0
    assert lib.dmb_conv3d_k3_bnstats_partials(4, 32, 64, 48, 136, 240) == 0     # Co != 32
