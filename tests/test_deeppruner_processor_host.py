"""DeepPruner's cost processor on the CPU: keys and shapes against the real reference's recording
(tests/golden/deeppruner_processor.npz, scripts/gen_golden_deeppruner_processor.py), construction from the reference's config,
the recording against the FP64 restatement (tests/_deeppruner_processor_ref.py), the conditions on the test inputs, the refusals of
the two entry points of csrc/deeppruner_heads.hip and of the modules, and the registries that stay as they were."""
import ctypes
import inspect
import json
import os

import pytest
import torch

from densematchingbenchmark_amd import _lib, ops, ops_deeppruner
from densematchingbenchmark_amd.config import Config
from densematchingbenchmark_amd.modeling.stereo.cost_processors.DeepPruner import ConfidenceRangePredictor, DeepPrunerProcessor
from densematchingbenchmark_amd.modeling.stereo.cost_processors.aggregators import DeepPrunerAggregator
from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils import HWHourglass
from densematchingbenchmark_amd.modeling.stereo.layers import SmallConv5x5
from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers import HeadConv3d
from tests import _deeppruner_processor_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = 100001, 100002


def _settings(rel="configs/DeepPruner/scene_flow_4x.py"):
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as fp:
        return Config(json.load(fp)[rel]["settings"])


def _cfg(C, P, N):
    return Config(dict(model=dict(batch_norm=True, cost_processor=dict(
        type="DeepPruner", patch_match_disparity_sample_number=P, uniform_disparity_sample_number=N,
        confidence_range_predictor=dict(in_planes=2 * C + 1, hourglass_in_planes=16),
        cost_aggregator=dict(type="DeepPruner", in_planes=2 * C + 2 * P + 1, hourglass_in_planes=16)))))


def _keys_and_shapes(module):
    sd = module.state_dict()
    return list(sd), [",".join(str(s) for s in t.shape) for t in sd.values()]


def test_state_dict_keys_and_shapes_equal_the_recording():
    z = R.recording()
    (B, C, P, N, H, W), _ = R.CASES["a"]                       # the case the recording took its key lists from
    ref = R.processor("a")
    for tag, hip, mine in (("processor", DeepPrunerProcessor(_cfg(C, P, N)), ref),
                           ("predictor", ConfidenceRangePredictor(2 * C + 1, 16, P), ref.confidence_range_predictor)):
        keys, shapes = [str(k) for k in z[tag + "/keys"]], [str(s) for s in z[tag + "/shapes"]]
        assert _keys_and_shapes(hip) == (keys, shapes), tag
        assert _keys_and_shapes(mine) == (keys, shapes), tag
        hip.load_state_dict(mine.state_dict(), strict=True)     # a seeded reference-style state_dict loads strictly
    assert len(z["processor/keys"]) == 258
    assert {"confidence_range_predictor.dres0.0.0.weight", "confidence_range_predictor.min_disparity_predictor.0.conv3_d.1.running_var",
            "confidence_range_predictor.max_disparity_predictor.2.weight", "confidence_range_predictor.min_disparity_conv.0.bias",
            "confidence_range_predictor.max_disparity_feature_conv.1.running_mean", "cost_aggregator.classify.1.weight",
            "disparity_conv.0.weight", "disparity_feature_conv.1.num_batches_tracked"} <= set(str(k) for k in z["processor/keys"])
    # the same 258 names at any sample counts
    for name in ("b", "c"):
        (B, C, P, N, H, W), _ = R.CASES[name]
        hip = DeepPrunerProcessor(_cfg(C, P, N))
        assert list(hip.state_dict()) == [str(k) for k in z["processor/keys"]]
        hip.load_state_dict(R.processor(name).state_dict(), strict=True)


def test_construction_from_the_reference_config():
    cfg = _settings()
    node = cfg.model.cost_processor.confidence_range_predictor
    assert dict(node) == dict(in_planes=65, hourglass_in_planes=16)
    proc = DeepPrunerProcessor(cfg)
    # the node is updated in place, as the reference does (DeepPruner.py:167-172)
    assert dict(node) == dict(in_planes=65, hourglass_in_planes=16, disparity_sample_number=14, batch_norm=True)
    assert proc.confidence_range_predictor_args is node
    assert proc.patch_match_disparity_sample_number == 14 and proc.uniform_disparity_sample_number == 9 and proc.batch_norm is True
    crp = proc.confidence_range_predictor
    assert (crp.in_planes, crp.hourglass_in_planes, crp.disparity_sample_number, crp.batch_norm) == (65, 16, 14, True)
    assert crp.dres0[0][0].in_channels == 65 and proc.cost_aggregator.dres0[0][0].in_channels == 93
    assert type(proc.cost_aggregator) is DeepPrunerAggregator and proc.cost_aggregator.in_planes == 93
    for branch in (crp.min_disparity_predictor, crp.max_disparity_predictor):
        assert isinstance(branch[0], HWHourglass) and branch[1][0].out_channels == 32 and type(branch[2]) is HeadConv3d
    for unit, (ci, has_bn) in ((crp.min_disparity_conv, (1, False)), (crp.max_disparity_conv, (1, False)),
                               (proc.disparity_conv, (1, False)), (crp.min_disparity_feature_conv, (14, True)),
                               (crp.max_disparity_feature_conv, (14, True)), (proc.disparity_feature_conv, (9, True))):
        assert type(unit) is SmallConv5x5 and unit.has_bn == has_bn and unit[0].in_channels == unit[0].out_channels == ci
        assert unit[0].kernel_size == (5, 5) and unit[0].padding == (2, 2) and unit[0].bias is not None
    assert len(proc.state_dict()) == 258 and len(DeepPrunerProcessor(_settings("configs/DeepPruner/scene_flow_8x.py")).state_dict()) == 258


def test_recording_lies_on_the_fp64_restatement():
    """A condition, not a tolerance (as test_restatement_in_fp64_lies_on_the_recording of the aggregator): a wrong tap, key or
    stage moves an output by its own magnitude, FP32 rounding by about 1e-5 of it at most."""
    z = R.recording()
    for name in R.CASES:
        f64 = R.fp64_outputs(name)
        for key in R.COSTS + R.OUTPUTS:
            rec = torch.from_numpy(z["%s/%s" % (name, key)]).double()
            assert rec.shape == f64[key].shape and torch.isfinite(rec).all(), (name, key)
            scale, err = f64[key].abs().max().item(), (rec - f64[key]).abs().max().item()
            print("%s %s: max|out| %.4g  max|recording - fp64| %.3g" % (name, key, scale, err))
            assert scale > 0.1 and err <= 1e-3 * scale, (name, key, err, scale)


def test_conditions_on_the_test_inputs():
    """Every disparity output is non-zero everywhere and every feature output on at least 30 % of its elements (a ReLU that
    swallowed a map would make every comparison of it pass); the warp's mask takes both branches."""
    z = R.recording()
    for name, ((B, C, P, N, H, W), _) in R.CASES.items():
        left, right, pre, post = R.case_inputs(name)
        assert pre.shape == (B, P, H, W) and post.shape == (B, N, H, W) and (pre[:, 1:] >= pre[:, :-1]).all()
        kept = (R.raw_volume(left, right, pre)[:, C:2 * C] > 0).float().mean().item()
        assert 0.3 <= kept <= 0.5, (name, kept)
        for key in R.OUTPUTS:
            share = (torch.from_numpy(z["%s/%s" % (name, key)]) != 0).float().mean().item()
            print("%s %s: non-zero on %.1f %%" % (name, key, 100 * share))
            assert share == 1.0 if "disparity" in key else share >= 0.3, (name, key, share)
        assert z[name + "/post/disparity"].shape == (B, 1, 2 * H, 2 * W) and z[name + "/post/feature"].shape == (B, N, 2 * H, 2 * W)


def _fake():
    """A non-NULL host address: the entry points must refuse before any device call, so it is never dereferenced."""
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def test_entry_points_validate_before_any_device_call():
    lib = _lib.load()
    keep, p = _fake()
    vol, conv = lib.dmb_deeppruner_volume_f32, lib.dmb_conv2d_k5_small_f32
    assert vol(None, None, None, None, None, None, 1, 4, 3, 8, 8, 0, None) == EINVAL
    assert b"deeppruner_volume" in lib.dmb_last_error()
    for args in ((None, p, p, None, None, p, 1, 4, 3, 8, 8, 0), (p, p, p, None, None, None, 1, 4, 3, 8, 8, 0),
                 (p, p, None, None, None, p, 1, 4, 3, 8, 8, 0), (p, p, p, None, None, p, 0, 4, 3, 8, 8, 0),
                 (p, p, p, None, None, p, 1, 0, 3, 8, 8, 0), (p, p, p, None, None, p, 1, 4, 0, 8, 8, 0),
                 (p, p, p, None, None, p, 1, 4, 3, -1, 8, 0), (p, p, p, None, None, p, 1, 4, 3, 8, 0, 0),
                 (p, p, p, None, None, p, 1, 4, 3, 8, 8, -1), (p, p, p, p, None, p, 1, 4, 3, 8, 8, 2),
                 (p, p, p, None, None, p, 1, 4, 3, 8, 8, 2), (p, p, p, p, p, p, 1, 4, 3, 8, 8, 0)):
        assert vol(*args, None) == EINVAL, args
        assert b"deeppruner_volume" in lib.dmb_last_error()
    for args in ((p, p, p, p, p, p, 1, 4, 3, 8, 8, 86), (p, p, p, None, None, p, 1, 4, 1, 8, 8, 0),
                 (p, p, p, None, None, p, 1, 4, 3, 1, 8, 0), (p, p, p, p, p, p, 1, 4, 3, 8, 1, 2)):
        assert vol(*args, None) == EUNSUPPORTED, args
        assert b"deeppruner_volume" in lib.dmb_last_error()
    assert conv(None, None, None, None, None, 1, 1, 1, 8, 8, 0, None) == EINVAL
    assert b"conv2d_k5_small" in lib.dmb_last_error()
    for args in ((None, p, None, None, p, 1, 4, 4, 8, 8, 0), (p, None, None, None, p, 1, 4, 4, 8, 8, 0),
                 (p, p, None, None, None, 1, 4, 4, 8, 8, 0), (p, p, None, None, p, 0, 4, 4, 8, 8, 0),
                 (p, p, None, None, p, 1, 4, 4, 0, 8, 0), (p, p, None, None, p, 1, 4, 4, 8, -3, 1),
                 (p, p, None, None, p, 1, -1, 4, 8, 8, 1), (p, p, None, None, p, 1, 4, -1, 8, 8, 1)):
        assert conv(*args, None) == EINVAL, args
        assert b"conv2d_k5_small" in lib.dmb_last_error()
    for Ci, Co in ((0, 4), (4, 0), (17, 4), (4, 17), (17, 17)):
        assert conv(p, p, p, p, p, 1, Ci, Co, 8, 8, 1, None) == EUNSUPPORTED, (Ci, Co)
        assert b"conv2d_k5_small" in lib.dmb_last_error()
    assert lib.dmb_abi_version() == _lib.ABI_VERSION
    del keep


def test_what_must_not_change():
    from densematchingbenchmark_amd.modeling import build_model
    from densematchingbenchmark_amd.modeling.stereo.cost_processors import PROCESSORS, build_cost_processor
    from densematchingbenchmark_amd.modeling.stereo.layers import FusedConv3d, bn_relu_conv  # noqa: F401
    cfg = _settings()
    assert set(PROCESSORS) == {'Difference', 'Concatenation', 'Correlation'}
    with pytest.raises(NotImplementedError):
        build_cost_processor(cfg)
    with pytest.raises(NotImplementedError):
        build_model(cfg, backbone=None)
    with pytest.raises(NotImplementedError):
        bn_relu_conv(True, 4, 4, kernel_size=5, padding=2)
    # the new launching wrappers live next to ops, not in it, and allocate through the module's own ``torch``
    assert not hasattr(ops, "deeppruner_volume") and not hasattr(ops, "conv2d_k5_small")
    assert ops_deeppruner.torch is torch
    for fn in (ops_deeppruner.deeppruner_volume, ops_deeppruner.conv2d_k5_small):
        src = inspect.getsource(fn)
        assert 'launch("dmb_' in src and "torch.empty(" in src and "empty_like" not in src and "new_empty" not in src
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    for bad in ((0, 4), (4, 0), (17, 4), (4, 17)):
        with pytest.raises(NotImplementedError):
            SmallConv5x5(True, *bad)


def test_training_and_gradients_are_refused():
    (B, C, P, N, H, W), _ = R.CASES["c"]
    proc = DeepPrunerProcessor(_cfg(C, P, N)).eval()
    left, right, pre, post = R.case_inputs("c")
    feat = torch.zeros((B, P, H, W))
    with pytest.raises(NotImplementedError, match="no backward"):
        proc("pre", left, right, pre)                           # eval(), but grad mode on and the parameters require grad
    with pytest.raises(NotImplementedError, match="no backward"):
        proc.train()("pre", left, right, pre)
    with pytest.raises(NotImplementedError, match="no backward"):
        with torch.no_grad():
            proc("post", left, right, post, feat, feat)         # still train()
    proc.eval().requires_grad_(False)
    for stage, args in (("pre", (left.clone().requires_grad_(), right, pre)), ("pre", (left, right, pre.clone().requires_grad_())),
                        ("post", (left, right, post, feat.clone().requires_grad_(), feat))):
        with pytest.raises(NotImplementedError, match="no backward"):
            proc(stage, *args)
    crp = proc.confidence_range_predictor
    raw = torch.zeros((B, 2 * C + 1, P, H, W))
    with pytest.raises(NotImplementedError, match="no backward"):
        crp(raw.clone().requires_grad_(), pre)
    with pytest.raises(NotImplementedError, match="no backward"):
        crp.range_costs(raw.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="no backward"):
        crp.heads(pre, pre.clone().requires_grad_(), pre)
    with pytest.raises(NotImplementedError, match="no backward"):
        crp.train()(raw, pre)
    unit = SmallConv5x5(True, 3, 3).eval()
    with pytest.raises(NotImplementedError, match="no backward"):
        unit(torch.zeros((1, 3, 4, 4)))                         # its own parameters require gradients
    with pytest.raises(NotImplementedError, match="no backward"):
        unit.requires_grad_(False).train()(torch.zeros((1, 3, 4, 4)))
