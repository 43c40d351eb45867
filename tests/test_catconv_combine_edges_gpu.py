"""The combining pass of the volume-free first layer (csrc/catconv.hip: catconv_combine_kernel<false> for the columns no mask band
reaches, <true> for the columns next to the band) at the shapes where its thread -> (row, column quad, plane range) mapping meets
its edges, bit for bit.

Two references:
  * the entry point itself, dmb_catconv_combine_f32, on random maps against its specification written out in torch (the header's
    and the kernel's comment: per element a selection between FM, the band word and zero, one addition f + g, one scale / shift,
    the activation; planes 0 and D - 1 summed from the per-dz maps).  The scales are powers of two, so the kernel's single fused
    multiply-add rounds exactly like the reference's separate multiply and add ((f + g) * 2^k is exact): ``torch.equal``, no
    tolerance.  Every map holds random values everywhere the kernel may read, so a wrong column, plane or band word shows.
  * the whole first layer, ``ops.catconv_first``, against the unfused form the existing tests use -- F.conv3d in FP64 on the oracle's
    concatenation volume -- with their bound of 2e-5 (another grouping of the same FP32 products: not the same bits).
Shapes: W = D + 8, where the near kernel owns every column quad but the last; widths that are no multiple of 16 (the near / far
split at 64 bytes leaves the far kernel 4, 8, 12 or 20 columns); D = 4 (one plane per thread of the near kernel's four plane
ranges: the border planes ARE the range); two batch items."""
import math

import pytest
import torch
import torch.nn.functional as F

from densematchingbenchmark_amd import ops
from densematchingbenchmark_amd._lib import launch
from oracle import dmb_oracle as O

pytestmark = pytest.mark.gpu

# (B, Co, D, H, W)
SHAPES = {"w_is_d_plus_8": (2, 4, 8, 3, 16), "w20_d12": (1, 3, 12, 2, 20), "w36_d12": (2, 2, 12, 3, 36), "w12_d4": (1, 5, 4, 2, 12),
          "w44_d16": (1, 2, 16, 2, 44), "w72_d48": (1, 2, 48, 1, 72)}


def _spec(FA, HC, FM, BAND, GM, GB, scale, shift, D, relu):
    """out[b, co, z, y, x] of include/dmb_hip.h (dmb_catconv_combine_f32), elementwise in FP32 on the CPU."""
    B, CA, H, W = FA.shape
    Co = FM.shape[1]
    x = torch.arange(W)
    out = torch.empty((B, Co, D, H, W))
    zero = torch.zeros(())
    for z in range(D):
        u = x - z
        if 0 < z < D - 1:
            f = FM
            g = GM[..., 4 + u.clamp(min=-4)]
        else:
            d0 = 1 if z == 0 else 0       # taps dz = 1, 2 on plane 0; dz = 0, 1 on plane D - 1
            f = FA[:, d0 * Co:(d0 + 1) * Co] + FA[:, (d0 + 1) * Co:(d0 + 2) * Co]
            n0, n1 = (u, u - 1) if z == 0 else (u + 1, u)

            def hc(dz, n):
                return torch.where(n >= -4, HC[:, dz * Co:(dz + 1) * Co][..., (4 + n).clamp(min=0)], zero)
            g = hc(d0, n0) + hc(d0 + 1, n1)
        band = BAND[:, :, :, z, :][..., (u + 2).clamp(0, 3)]
        f = torch.where(u >= 2, f, torch.where(u >= -2, band, zero))
        g = g.clone()
        g[..., W - 1] = GB[:, :, :, z]
        v = (f + g) * scale.view(1, Co, 1, 1) + shift.view(1, Co, 1, 1)
        out[:, :, z] = v.clamp(min=0.0) if relu else v
    return out


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_combine_equals_its_specification(dev, name, relu):
    B, Co, D, H, W = SHAPES[name]
    CA = 3 * Co
    g = torch.Generator().manual_seed(W * 100 + D)
    FA, HC = torch.randn((B, CA, H, W), generator=g), torch.randn((B, CA, H, W + 4), generator=g)
    FM, GM = torch.randn((B, Co, H, W), generator=g), torch.randn((B, Co, H, W + 4), generator=g)
    BAND, GB = torch.randn((B, Co, H, D, 4), generator=g), torch.randn((B, Co, H, D), generator=g)
    scale = torch.tensor([2.0 ** (i % 5 - 2) * (-1.0 if i % 3 == 2 else 1.0) for i in range(Co)])
    shift = torch.randn(Co, generator=g)
    out = torch.full((B, Co, D, H, W), float("nan"), device=dev)
    launch("dmb_catconv_combine_f32", FA.to(dev), HC.to(dev), FM.to(dev), BAND.to(dev), GM.to(dev), GB.to(dev), scale.to(dev),
           shift.to(dev), out, B, Co, CA, D, H, W, int(relu))
    want = _spec(FA, HC, FM, BAND, GM, GB, scale, shift, D, relu)
    got = out.cpu()
    assert bool(torch.isfinite(got).all()), "%d elements were not written" % int((~torch.isfinite(got)).sum())
    bad = (got != want).nonzero()
    assert bad.numel() == 0, "%d elements differ, first at (b, co, z, y, x) = %s: %r vs %r" % (
        bad.shape[0], tuple(bad[0].tolist()), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())


@pytest.mark.parametrize("B,C,D,H,W", [(2, 8, 8, 5, 16), (1, 8, 12, 4, 36), (1, 6, 12, 3, 20)])
def test_first_layer_at_the_edge_widths(dev, single_chain, B, C, D, H, W):
    g = torch.Generator().manual_seed(W)
    L, R = torch.randn((B, C, H, W), generator=g), torch.randn((B, C, H, W), generator=g)
    w = torch.randn((32, 2 * C, 3, 3, 3), generator=g) / math.sqrt(2 * C * 27 / 8)
    sc, sh = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.2
    assert ops.catconv_applicable(L.to(dev), R.to(dev), ops.disp_index_list(D, 0, 1), 32)
    ref = F.relu(F.conv3d(O.cat_fms(L, R, D, 0, 1).double(), w.double(), None, padding=1) * sc.double().view(1, -1, 1, 1, 1)
                 + sh.double().view(1, -1, 1, 1, 1))
    got = ops.catconv_first(L.to(dev), R.to(dev), D, ops.catconv_pack(w.to(dev)), sc.to(dev), sh.to(dev), True).cpu()
    err = (got.double() - ref).abs().max().item()
    print("W = %d, D = %d: max |first layer - fp64| = %.3e" % (W, D, err))
    assert got.shape == ref.shape and err <= 2e-5
