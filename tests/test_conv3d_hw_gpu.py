"""The (y, x)-strided 3-D convolution family (csrc/conv3d_hw.hip) on the MI355X against F.conv3d / F.conv_transpose3d on the CPU.

Inputs as in tests/test_kernels_gpu.py: |x| ~ 1, weights / sqrt(K) (K = Ci * 27, for the transposed layer the Ci * 27 / 4 taps that
reach an output voxel on average), a random affine.  Every case runs three ways: plain; affine + residual + ReLU; ReLU 'pre' +
residual.  Bounds: 2e-5 for Ci <= 64 (the project's figure for a Ci * 27 chain at unit scale); for Ci = 128 the chain is twice as
long and rounding grows with its square root: 2e-5 * sqrt(2).

Also: the stride-(1, 2, 2) result equals the single-chain stride-1 result at even (y, x) BIT FOR BIT (same chain, same stream,
padding taps add exact zeros), batch invariance bit for bit, run-to-run identity, and the refusals.

Measured maxima on an MI355X: see docs/design/15-deeppruner-aggregator.md."""
import math

import pytest
import torch
import torch.nn.functional as F

from densematchingbenchmark_amd import _lib, ops

pytestmark = pytest.mark.gpu
HW = (1, 2, 2)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.5 + torch.rand(C, generator=g), torch.rand(C, generator=g) - 0.5


def _bound(Ci):
    return 2e-5 * (math.sqrt(2.0) if Ci > 64 else 1.0)


def _three_ways(run, raw, Co, Ci, dev, what):
    """``run(scale, shift, residual, relu)`` -> device tensor; ``raw``: the CPU convolution without epilogue."""
    sc, sh = _affine(Co, 7)
    res = _rand(raw.shape, 8)
    aff = raw * sc.view(1, -1, 1, 1, 1) + sh.view(1, -1, 1, 1, 1)
    wants = (("plain", (None, None, None, False), raw),
             ("affine+residual+relu", (sc.to(dev), sh.to(dev), res.to(dev), True), F.relu(aff + res)),
             ("relu-pre+residual", (None, None, res.to(dev), "pre"), F.relu(raw) + res))
    for tag, args, want in wants:
        got = run(*args).cpu()
        assert got.shape == want.shape, (what, tag, got.shape, want.shape)
        err = (got - want).abs().max().item()
        print("%s %s: max err %.3g (bound %.3g)" % (what, tag, err, _bound(Ci)))
        assert torch.isfinite(got).all() and err <= _bound(Ci), (what, tag, err)


@pytest.mark.parametrize("Ci,Co", [(16, 32), (32, 64), (64, 128), (5, 32), (20, 64), (12, 16)])
@pytest.mark.parametrize("shape", [(2, 3, 10, 70), (1, 1, 9, 13), (1, 5, 8, 96), (2, 2, 1, 48), (1, 4, 17, 30), (1, 3, 6, 1)])
def test_conv3d_stride_122(dev, Ci, Co, shape):
    B, D, H, W = shape
    x = _rand((B, Ci, D, H, W), 5)
    w = _rand((Co, Ci, 3, 3, 3), 6, 1.0 / math.sqrt(Ci * 27))
    raw = F.conv3d(x, w, None, stride=HW, padding=1)
    xd, wp = x.to(dev), ops.pack_conv3d_weights(w.to(dev))
    _three_ways(lambda sc, sh, res, relu: ops.conv3d_k3(xd, wp, Co, sc, sh, res, HW, relu), raw, Co, Ci, dev,
                "conv s122 %d->%d %s" % (Ci, Co, shape))


@pytest.mark.parametrize("Ci,Co", [(128, 64), (64, 32), (32, 16), (9, 16), (20, 32)])
@pytest.mark.parametrize("shape", [(2, 3, 5, 35), (1, 1, 6, 61), (1, 5, 7, 64), (2, 3, 1, 30), (1, 14, 2, 3)])
def test_deconv3d_stride_122(dev, Ci, Co, shape):
    B, D, H, W = shape
    x = _rand((B, Ci, D, H, W), 9)
    w = _rand((Ci, Co, 3, 3, 3), 10, 1.0 / math.sqrt(Ci * 27 / 4))
    raw = F.conv_transpose3d(x, w, None, stride=HW, padding=1, output_padding=(0, 1, 1))
    assert raw.shape == (B, Co, D, 2 * H, 2 * W)
    xd, wp = x.to(dev), ops.pack_deconv3d_weights(w.to(dev))
    _three_ways(lambda sc, sh, res, relu: ops.deconv3d_k3s2(xd, wp, Co, sc, sh, res, relu, stride=HW), raw, Co, Ci, dev,
                "deconv s122 %d->%d %s" % (Ci, Co, shape))


@pytest.mark.parametrize("Ci,Co", [(32, 16), (5, 16)])
@pytest.mark.parametrize("shape", [(2, 3, 5, 48), (1, 1, 9, 13), (1, 14, 6, 70)])
def test_conv3d_stride_1_to_16_channels(dev, Ci, Co, shape):
    B, D, H, W = shape
    x = _rand((B, Ci, D, H, W), 13)
    w = _rand((Co, Ci, 3, 3, 3), 14, 1.0 / math.sqrt(Ci * 27))
    raw = F.conv3d(x, w, None, stride=1, padding=1)
    xd, wp = x.to(dev), ops.pack_conv3d_weights(w.to(dev))
    _three_ways(lambda sc, sh, res, relu: ops.conv3d_k3(xd, wp, Co, sc, sh, res, 1, relu), raw, Co, Ci, dev,
                "conv s1 %d->%d %s" % (Ci, Co, shape))
    # (1, 1, 1) means 1
    assert torch.equal(ops.conv3d_k3(xd, wp, Co, stride=(1, 1, 1)), ops.conv3d_k3(xd, wp, Co, stride=1))


@pytest.mark.parametrize("Ci,Co,shape", [(16, 32, (2, 3, 10, 70)), (32, 64, (1, 5, 8, 96)), (64, 128, (1, 4, 17, 30)),
                                         (20, 64, (1, 1, 9, 13)), (5, 32, (2, 2, 1, 48))])
def test_stride_122_equals_stride_1_at_even_positions_bit_for_bit(dev, Ci, Co, shape):
    """No tolerance: one fma chain per voxel in the packed stream's order in both kernels; the taps that fall into the padding
    add exact zeros in both."""
    B, D, H, W = shape
    x = _rand((B, Ci, D, H, W), 21).to(dev)
    wp = ops.pack_conv3d_weights(_rand((Co, Ci, 3, 3, 3), 22, 1.0 / math.sqrt(Ci * 27)).to(dev))
    sc, sh = (t.to(dev) for t in _affine(Co, 23))
    before = ops.split_k()
    ops.set_split_k(False)
    try:
        for args in ((None, None, None), (sc, sh, None)):
            relu = args[0] is not None
            strided = ops.conv3d_k3(x, wp, Co, *args, stride=HW, relu=relu)
            dense = ops.conv3d_k3(x, wp, Co, *args, stride=1, relu=relu)
            assert strided.shape == dense[..., ::2, ::2].shape
            assert torch.equal(strided, dense[..., ::2, ::2].contiguous()), (Ci, Co, shape, relu)
            assert torch.equal(ops.conv3d_k3(x, wp, Co, *args, stride=(2, 2, 2), relu=relu), ops.conv3d_k3(x, wp, Co, *args, stride=2, relu=relu))
    finally:
        ops.set_split_k(before)


def _kernels(dev):
    """(name, run(x) -> y, input shape for batch 2) of the three kernel forms on fixed weights."""
    out = []
    for name, Ci, Co, shape in (("conv_s122", 20, 64, (2, 20, 3, 9, 34)), ("conv_s1_co16", 32, 16, (2, 32, 3, 5, 40)),
                                ("deconv_s122", 64, 32, (2, 64, 3, 5, 19))):
        transposed = name.startswith("deconv")
        w = _rand((Ci, Co, 3, 3, 3) if transposed else (Co, Ci, 3, 3, 3), 31, 1.0 / math.sqrt(Ci * 27)).to(dev)
        sc, sh = (t.to(dev) for t in _affine(Co, 32))
        if transposed:
            wp = ops.pack_deconv3d_weights(w)
            run = (lambda wp, Co, sc, sh: lambda x: ops.deconv3d_k3s2(x, wp, Co, sc, sh, None, True, stride=HW))(wp, Co, sc, sh)
        else:
            wp = ops.pack_conv3d_weights(w)
            stride = HW if name == "conv_s122" else 1
            run = (lambda wp, Co, sc, sh, stride: lambda x: ops.conv3d_k3(x, wp, Co, sc, sh, None, stride, True))(wp, Co, sc, sh, stride)
        out.append((name, run, shape))
    return out


def test_batch_invariance_and_run_to_run_identity(dev):
    kernels = _kernels(dev)
    for name, run, shape in kernels:           # default policy: two identical calls are bit-identical
        x = _rand(shape, 33).to(dev)
        assert torch.equal(run(x), run(x)), name
    before = ops.split_k()
    ops.set_split_k(False)
    try:
        for name, run, shape in kernels:       # single-chain policy: item 1 of a batch of 2 equals the item run alone
            x = _rand(shape, 33).to(dev)
            both, alone = run(x), run(x[1:2].contiguous())
            assert torch.equal(both[1:2], alone), name
    finally:
        ops.set_split_k(before)


def test_refusals(dev):
    x = torch.zeros((1, 16, 2, 8, 8), device=dev)
    w32 = ops.pack_conv3d_weights(torch.zeros((32, 16, 3, 3, 3), device=dev))
    w8 = ops.pack_conv3d_weights(torch.zeros((8, 16, 3, 3, 3), device=dev))
    with pytest.raises(_lib.DmbLibraryError, match="100002"):
        ops.conv3d_k3(x, w8, 8, stride=HW)
    with pytest.raises(_lib.DmbLibraryError, match="stride"):
        ops.conv3d_k3(x, w32, 32, stride=(2, 1, 2))
    with pytest.raises(_lib.DmbLibraryError, match="residual shape"):
        ops.conv3d_k3(x, w32, 32, residual=torch.zeros((1, 32, 2, 8, 8), device=dev), stride=HW)
    with pytest.raises(_lib.DmbLibraryError, match="packed weights"):
        ops.conv3d_k3(x, w32, 64, stride=HW)
    with pytest.raises(_lib.DmbLibraryError, match="scale"):
        ops.conv3d_k3(x, w32, 32, scale=torch.ones(16, device=dev), stride=HW)
    with pytest.raises(_lib.DmbLibraryError, match="out must be"):
        ops.conv3d_k3(x, w32, 32, stride=HW, out=torch.zeros((1, 32, 2, 8, 8), device=dev))
    wd = ops.pack_deconv3d_weights(torch.zeros((16, 32, 3, 3, 3), device=dev))
    with pytest.raises(_lib.DmbLibraryError, match="out_width"):
        ops.deconv3d_k3s2(x, wd, 32, stride=HW, out_width=12)
    with pytest.raises(_lib.DmbLibraryError, match="workspace"):
        ops.deconv3d_k3s2(x, wd, 32, stride=HW, workspace=None)
    with pytest.raises(_lib.DmbLibraryError, match="residual shape"):
        ops.deconv3d_k3s2(x, wd, 32, residual=torch.zeros((1, 32, 4, 16, 16), device=dev), stride=HW)
    with pytest.raises(_lib.DmbLibraryError, match="stride"):
        ops.deconv3d_k3s2(x, wd, 32, stride=(2, 1, 2))
    wd128 = ops.pack_deconv3d_weights(torch.zeros((16, 128, 3, 3, 3), device=dev))
    with pytest.raises(_lib.DmbLibraryError, match="100002"):
        ops.deconv3d_k3s2(x, wd128, 128, stride=HW)
    # out= is honoured and written in full
    out = torch.full((1, 32, 2, 16, 16), float("nan"), device=dev)
    assert ops.deconv3d_k3s2(x, wd, 32, stride=HW, out=out) is out and bool((out == 0).all())
