"""DeepPruner's refinement and backbones on the MI355X against the real reference's recording
(tests/golden/deeppruner_features.npz) and the restatement (tests/_deeppruner_features_ref.py) in FP64.

The contract (``_check``, the aggregator's: docs/design/15-deeppruner-aggregator.md): with fp64 = the restatement in FP64,
e_ref = |recording - fp64| and e_hip = |hip - fp64|,
    max e_hip <= max(2e-5 * max(1, max|fp64|), FACTOR * max e_ref)     and     mean e_hip <= 2 * mean e_ref,
FACTOR = 1.25, for every up-sampled map of the three refinement cases and, on the recorded strided sub-samples, for the feature
and every low-level map of the two backbones.  Measured on an MI355X: see the tables of docs/design/17-deeppruner-features.md."""
import pytest
import torch

from densematchingbenchmark_amd.modeling.stereo.backbones import DeepPrunerBestBackbone, DeepPrunerFastBackbone
from densematchingbenchmark_amd.modeling.stereo.disp_refinement import DeepPrunerRefinement
from tests import _deeppruner_features_ref as R

pytestmark = pytest.mark.gpu
FACTOR = 1.25
HIP = {"best": DeepPrunerBestBackbone, "fast": DeepPrunerFastBackbone}


def _check(hip, ref32, fp64, what, factor=FACTOR):
    hip, fp64 = hip.double().cpu(), fp64.double().cpu()
    assert hip.shape == fp64.shape, (what, hip.shape, fp64.shape)
    assert torch.isfinite(hip).all(), what
    d_hip, d_ref = (hip - fp64).abs(), (ref32.double().cpu() - fp64).abs()
    e_hip, m_hip, scale = d_hip.max().item(), d_hip.mean().item(), max(1.0, fp64.abs().max().item())
    e_ref, m_ref = d_ref.max().item(), d_ref.mean().item()
    print("%s: max|fp64| %.4g  e_hip %.4g e_ref %.4g (ratio %.3g)  mean_hip %.4g mean_ref %.4g (ratio %.3g)"
          % (what, scale, e_hip, e_ref, e_hip / max(e_ref, 1e-30), m_hip, m_ref, m_hip / max(m_ref, 1e-30)))
    assert e_hip <= max(2e-5 * scale, factor * e_ref), (what, e_hip, e_ref)
    assert m_hip <= 2.0 * m_ref, (what, m_hip, m_ref)


def _refinement(dev, name):
    (planes, num, _, _), _ = R.REFINE_CASES[name]
    hip = DeepPrunerRefinement(list(planes), True, num)
    hip.load_state_dict(R.refinement(name).state_dict(), strict=True)
    return hip.to(dev).eval()


@pytest.mark.parametrize("name", list(R.REFINE_CASES))
def test_refinement_against_the_recording(dev, name):
    z = R.recording()
    (planes, num, B, (H, W)), _ = R.REFINE_CASES[name]
    disps, fms = R.refine_inputs(name)
    d_dev, f_dev = [t.to(dev) for t in disps], [t.to(dev) for t in fms]
    kept = [t.clone() for t in f_dev]
    with torch.no_grad():
        got = _refinement(dev, name)(list(d_dev), f_dev)
    assert len(got) == num + 1 and got[-1] is d_dev[0]                      # reversed: the better map first, the input last
    assert all(torch.equal(a, b) for a, b in zip(kept, f_dev))              # low_ref_group_fms is not modified
    f64 = R.fp64_refinement(name)
    for i in range(num):
        up = got[num - 1 - i]
        assert up.shape == (B, 1, (H << i) * 2, (W << i) * 2)
        _check(up, torch.from_numpy(z["%s/up%d" % (name, i)]), f64[i][1], "%s up%d" % (name, i))


@pytest.mark.parametrize("name", list(R.BACKBONE_CASES))
def test_backbone_against_the_recording(dev, name):
    z = R.recording()
    hip = HIP[name]()
    hip.load_state_dict(R.backbone(name).state_dict(), strict=True)
    hip = hip.to(dev).eval()
    x = R.backbone_input(name).to(dev)
    with torch.no_grad():
        left, right = hip(x, x)
    lmaps, rmaps = R.flatten(left), R.flatten(right)
    assert isinstance(left, tuple) and isinstance(left[1], list) and len(lmaps) == len(R.BACKBONE_CASES[name][3])
    assert [list(m.shape) for m in lmaps] == z[name + "/full_shapes"].tolist()
    f64 = R.fp64_backbone(name)
    for i, (a, b, sub) in enumerate(zip(lmaps, rmaps, R.subsample(name, lmaps))):
        assert torch.equal(a, b), "the two views of one image differ: %s map %d" % (name, i)   # two streams, the same launches
        _check(sub, torch.from_numpy(z["%s/map%d" % (name, i)]), f64[i], "%s map%d" % (name, i))


def test_refinement_graph_replay_equals_eager_bit_for_bit(dev):
    name = "r8x"
    hip = _refinement(dev, name)
    disps, fms = R.refine_inputs(name)
    d_dev, f_dev = [t.to(dev) for t in disps], [t.to(dev) for t in fms]
    with torch.no_grad():
        eager = [t.clone() for t in hip(list(d_dev), f_dev)]               # (also fills the packed-weight caches before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = hip(list(d_dev), f_dev)
        for t in captured[:-1]:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert len(captured) == len(eager) == 3
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)


def test_classify_weight_changed_in_place_is_seen_by_the_next_call(dev):
    name = "rodd"
    hip = _refinement(dev, name)
    disps, fms = R.refine_inputs(name)
    d_dev, f_dev = [t.to(dev) for t in disps], [t.to(dev) for t in fms]
    with torch.no_grad():
        before = hip(list(d_dev), f_dev)[0].clone()
        hip.refine_blocks[0].classify.weight.mul_(-1.0)
        after = hip(list(d_dev), f_dev)[0]
        fresh = _refinement(dev, name)
        fresh.refine_blocks[0].classify.weight.mul_(-1.0)
        want = fresh(list(d_dev), f_dev)[0]
        # and a folded BatchNorm follows the same rule (param_state)
        hip.refine_blocks[0].conv[5][1].weight.mul_(0.5)
        fresh2 = _refinement(dev, name)
        fresh2.refine_blocks[0].classify.weight.mul_(-1.0)
        fresh2.refine_blocks[0].conv[5][1].weight.mul_(0.5)
        assert torch.equal(hip(list(d_dev), f_dev)[0], fresh2(list(d_dev), f_dev)[0])
    assert not torch.equal(before, after) and torch.equal(after, want)
