"""Badly conditioned values in the per-channel reducing kernels of norm.hip and in the statistics epilogue of the 3-D convolution.

The rest of the suite draws its operands from randn * O(1).  Here one launch sees channels whose mean is 100 or 1000 standard
deviations away, whose spread is tiny, which are constant, sparse, scaled by 1e4 or 1e-3, or whose FIRST element -- the pivot the
batch-statistics kernel subtracts -- is an outlier (tests/_values.py names them).  Every output is compared with an FP64 evaluation,
per channel, within 4x the distance of an FP32 evaluation of the same inputs (ATen's, or next to the case what stands in for it) plus
2e-6 of the channel's own range
(_values.check_per_channel).  relu=False throughout, so every element of every output is compared."""
import pytest
import torch

from tests import _values as V

pytestmark = pytest.mark.gpu


def _ops():
    from densematchingbenchmark_amd import ops

    return ops


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_batch_statistics(dev, case):
    """bn_train_stats (+ bn_act) and bn_train_fwd, with running buffers: mean, invstd, scale, shift, running_mean, running_var, y.
    Without affine parameters and running buffers the statistics are the same bits."""
    ops = _ops()
    k = V.bn_case(*case)
    c = k["c"].to(dev)
    gamma, beta = k["gamma"].to(dev), k["beta"].to(dev)
    rm, rv = k["rm0"].to(dev), k["rv0"].to(dev)
    mean, invstd, scale, shift = ops.bn_train_stats(c, gamma, beta, rm, rv, momentum=0.1, eps=1e-5)
    y = ops.bn_act(c, scale, shift, None, relu=False)
    got = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, running_mean=rm, running_var=rv, y=y)
    V.check_bn_forward(got, k["c"], k["gamma"], k["beta"], k["rm0"], k["rv0"], k["names"])
    rm, rv = k["rm0"].to(dev), k["rv0"].to(dev)
    y, mean, invstd, scale, shift = ops.bn_train_fwd(c, gamma, beta, rm, rv, None, 0.1, 1e-5, None, False)
    got = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, running_mean=rm, running_var=rv, y=y)
    V.check_bn_forward(got, k["c"], k["gamma"], k["beta"], k["rm0"], k["rv0"], k["names"])
    m0, i0, s0, h0 = ops.bn_train_stats(c, None, None, None, None, momentum=0.1, eps=1e-5)
    assert torch.equal(m0, mean) and torch.equal(i0, invstd) and torch.equal(s0, invstd)
    y0, m1, i1, _, _ = ops.bn_train_fwd(c, None, None, None, None, None, 0.1, 1e-5, None, False)
    assert torch.equal(m1, mean) and torch.equal(i1, invstd) and torch.equal(y0, ops.bn_act(c, s0, h0, None, relu=False))


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_bn_backward(dev, case):
    """bn_act_bwd in training mode on the statistics the forward kernel returned: dc, which scales with 1 / std, per channel; dgamma and
    dbeta, which do not scale with the input, per channel with the floor of the whole vector's range.  The yardstick is the FP64
    evaluation on FP32-stored statistics (_values.bn_backward_reference), not ATen's FP32 autograd: that one also sums in FP32 and
    is up to 6e-4 of the range off on ``tiny``, a bound that would let a wrong reduction through."""
    ops = _ops()
    k = V.bn_case(*case)
    ref64, _, stored = V.bn_backward_reference(k["c"], k["gamma"], k["beta"], k["dy"])
    c, dy = k["c"].to(dev), k["dy"].to(dev)
    mean, invstd, scale, shift = ops.bn_train_stats(c, k["gamma"].to(dev), k["beta"].to(dev), None, None, momentum=0.1, eps=1e-5)
    y = ops.bn_act(c, scale, shift, None, relu=False)
    dc, dgamma, dbeta, _ = ops.bn_act_bwd(dy, c, y, scale, shift, mean, invstd, relu=False, training=True)
    V.check_per_channel(dc, ref64["dc"], stored["dc"], "dc", k["names"])
    # a channel's sum may cancel to nothing: the floor is relative to the vector's range, the reference's error the channel's own
    for name, got in (("dgamma", dgamma), ("dbeta", dbeta)):
        V.check_per_channel(got, ref64[name], stored[name], name, k["names"], scale=ref64[name].abs().max().expand(len(k["names"])))


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_channel_dot(dev, case):
    """channel_dot with ``a`` from the distributions and ``g`` plain, per channel (the channels' sums differ by 1e7)."""
    ops = _ops()
    shape, first = case
    k = V.bn_case(*case)
    a = k["c"]
    g = V.mixed((shape[0], 1) + tuple(shape[2:]), 13, names=("plain",))[0]
    ref64 = (a.double() * g.double()).sum(dim=[0] + list(range(2, a.dim())))
    ref32 = (a * g).sum(dim=[0] + list(range(2, a.dim())))
    got = ops.channel_dot(a.to(dev), g.to(dev))
    V.check_per_channel(got, ref64, ref32, "channel_dot", k["names"])


@pytest.mark.parametrize("offset", V.EPILOGUE_OFFSETS)
@pytest.mark.parametrize("shape", V.EPILOGUE_SHAPES)
def test_statistics_from_the_convolution_epilogue(dev, shape, offset):
    """conv3d_k3_bnstats + bn_train_act through the real kernel, the raw output carrying a mean of about 0, 100 and 1000 standard
    deviations (_values.centre_tap_conv_inputs).  The reference is the FP64 batch normalisation of the raw output the kernel itself
    returned, the yardstick ATen's FP32 one of the same tensor."""
    ops = _ops()
    x, w = V.centre_tap_conv_inputs(shape, 32, offset, 131)
    fused = ops.conv3d_k3_bnstats(x.to(dev), ops.pack_conv3d_weights(w.to(dev)), 32)
    assert fused is not None
    raw, parts = fused
    gamma, beta, rm0, rv0 = V._vec(32, 2, 0.5, 1.0), V._vec(32, 3, 0.2), V._vec(32, 6, 0.1), V._vec(32, 7).abs() + 0.5
    rm, rv = rm0.to(dev), rv0.to(dev)
    y, mean, invstd, scale, shift = ops.bn_train_act(raw, parts, gamma.to(dev), beta.to(dev), rm, rv, None, 0.1, 1e-5, None, False)
    got = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, running_mean=rm, running_var=rv, y=y)
    V.check_bn_forward(got, raw.cpu(), gamma, beta, rm0, rv0, ["offset %g, channel %d" % (offset, ch) for ch in range(32)],
                       stored_y=[offset != 0.0] * 32)
    # (y by the stored (scale, shift) form, _values.STORAGE_BOUND_Y, at both offsets: at 2000 the rounding of shift puts 8 of the 64
    # channels at 5e-5 .. 1.3e-4 against 2e-5 .. 9e-5 allowed by ATen's y, and at 200 one channel of (2, 16, 6, 7, 24) at 7.53e-6
    # against 7.44e-6)
