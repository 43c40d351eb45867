"""DeepPruner's aggregator and HWHourglass on the MI355X against the real reference's recording
(tests/golden/deeppruner_aggregator.npz) and the restatement (tests/_hw_ref.py) in FP64.

The contract (``_check``): with fp64 = the restatement in FP64, e_ref = |recording - fp64| and e_hip = |hip - fp64|,
    max e_hip <= max(2e-5 * max(1, max|fp64|), 1.25 * max e_ref)     and     mean e_hip <= 2 * mean e_ref.
The floor is the project's single-layer tolerance at the output's scale; the mean gets a factor 2 over the reference's own error
because the single-chain sum of up to 3456 terms is compared with the CPU library's blocked sums and may carry more rounding --
more than that factor is not rounding.

Measured on an MI355X: see the table of docs/design/15-deeppruner-aggregator.md."""
import os

import numpy as np
import pytest
import torch

from densematchingbenchmark_amd.modeling.stereo.cost_processors.aggregators import DeepPrunerAggregator
from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils import HWHourglass
from tests import _hw_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "deeppruner_aggregator.npz")


def _check(hip, ref32, fp64, what):
    hip, ref32, fp64 = hip.double().cpu(), ref32.double().cpu(), fp64.double().cpu()
    assert hip.shape == fp64.shape, (what, hip.shape, fp64.shape)
    d_hip, d_ref = (hip - fp64).abs(), (ref32 - fp64).abs()
    e_hip, e_ref, m_hip, m_ref = d_hip.max().item(), d_ref.max().item(), d_hip.mean().item(), d_ref.mean().item()
    scale = max(1.0, fp64.abs().max().item())
    print("%s: max|fp64| %.4g  e_hip %.4g e_ref %.4g  mean_hip %.4g mean_ref %.4g" % (what, scale, e_hip, e_ref, m_hip, m_ref))
    assert torch.isfinite(hip).all(), what
    assert e_hip <= max(2e-5 * scale, 1.25 * e_ref), (what, e_hip, e_ref)
    assert m_hip <= 2.0 * m_ref, (what, m_hip, m_ref)


def _aggregator(dev, seed=R.WEIGHT_SEED, in_planes=R.IN_PLANES):
    return R.seeded_state(DeepPrunerAggregator(in_planes, R.HOURGLASS_IN_PLANES), seed).to(dev).eval()


def test_aggregator_against_reference_recording(dev):
    z = np.load(GOLDEN)
    agg = _aggregator(dev)
    for name in R.GOLDEN_CASES:
        x = R.golden_input(name)
        with torch.no_grad():
            out = agg(x.to(dev))
        assert isinstance(out, list) and len(out) == 1 and out[0].shape == (x.shape[0],) + tuple(x.shape[2:])
        _check(out[0], torch.from_numpy(z[name + "/out"]), R.fp64_output(name), "aggregator " + name)


def test_hourglass_against_reference_recording(dev):
    z = np.load(GOLDEN)
    hg = R.seeded_state(HWHourglass(R.HOURGLASS_IN_PLANES), R.WEIGHT_SEED + 1).to(dev).eval()
    for name in R.HOURGLASS_CASES:
        x = R.golden_input(name)
        with torch.no_grad():
            out = hg(x.to(dev))
        _check(out, torch.from_numpy(z[name + "/out"]), R.fp64_output(name), "hourglass " + name)
    # the fused caller's add: hourglass(x, skip=s) == hourglass(x) + s, one rounding apart at most
    x = R.golden_input("hg_a").to(dev)
    with torch.no_grad():
        assert torch.allclose(hg(x, skip=x), hg(x) + x, rtol=0, atol=1e-5)


def test_aggregator_at_config_width(dev):
    """in_planes = 93 (2 * 32 + 2 * 14 + 1) at [1, 93, 9, 24, 40]: the yardsticks run by stock torch on the device."""
    x = torch.randn((1, 93, 9, 24, 40), generator=torch.Generator().manual_seed(41))
    ref = R.seeded_state(R.DeepPrunerAggregator(93, 16), 43).eval()
    agg = _aggregator(dev, 43, 93)
    with torch.no_grad():
        out = agg(x.to(dev))[0]
        ref32 = ref.to(dev)(x.to(dev))[0]
        fp64 = ref.double()(x.to(dev).double())[0]
    _check(out, ref32, fp64, "aggregator 93 planes")


def test_graph_replay_equals_eager(dev):
    agg = _aggregator(dev)
    x = R.golden_input("b").to(dev)
    with torch.no_grad():
        eager = agg(x)[0].clone()
        static_x = x.clone()
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            agg(static_x)                                      # warm-up: packs and folds outside the capture
        torch.cuda.current_stream(dev).wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = agg(static_x)[0]
        static_x.copy_(torch.zeros_like(x))
        graph.replay()
        assert not torch.equal(static_out, eager)
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, eager)


def test_weight_updates_reach_the_next_output(dev):
    """The staleness rule (param_state.cached) through the new units: an in-place change or a reload is seen by the next call."""
    agg = _aggregator(dev)
    x = R.golden_input("a").to(dev)
    with torch.no_grad():
        first = agg(x)[0].clone()
        assert torch.equal(agg(x)[0], first)
        agg.dres2.conv2_a[0].weight.mul_(1.5)                  # a stride-(1, 2, 2) unit
        second = agg(x)[0].clone()
        assert not torch.equal(second, first)
        agg.dres2.conv3_d[1].running_var.add_(0.25)            # the folded BatchNorm of a transposed unit
        third = agg(x)[0].clone()
        assert not torch.equal(third, second)
        agg.dres1[1][0].weight.mul_(0.5)                       # the 32 -> 16 unit
        assert not torch.equal(agg(x)[0], third)
        R.seeded_state(agg, R.WEIGHT_SEED + 7)
        other = agg(x)[0].clone()
        want = R.seeded_state(R.DeepPrunerAggregator(R.IN_PLANES, R.HOURGLASS_IN_PLANES), R.WEIGHT_SEED + 7).double().eval()(x.cpu().double())[0]
        assert (other.cpu().double() - want).abs().max().item() <= 1e-3 * want.abs().max().item()
        R.seeded_state(agg, R.WEIGHT_SEED)
        assert torch.equal(agg(x)[0], first)


def test_training_and_gradients_are_refused(dev):
    agg = _aggregator(dev)
    x = R.golden_input("c").to(dev)
    with pytest.raises(NotImplementedError, match="no backward"):
        agg(x.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="no backward"):
        agg(x)                                                 # eval(), but grad mode on and the parameters require grad
    with pytest.raises(NotImplementedError, match="no backward"):
        agg.train()(x)
    hg = HWHourglass(16).to(dev).eval()
    with pytest.raises(NotImplementedError, match="no backward"):
        hg(torch.zeros((1, 16, 2, 8, 8), device=dev, requires_grad=True))
    with pytest.raises(ValueError, match="multiples of 8"):
        with torch.no_grad():
            hg(torch.zeros((1, 16, 2, 12, 8), device=dev))
