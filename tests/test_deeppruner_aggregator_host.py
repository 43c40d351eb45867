"""DeepPruner's aggregator on the CPU: keys and shapes against the real reference's recording
(tests/golden/deeppruner_aggregator.npz, scripts/gen_golden_deeppruner_aggregator.py), the builders, the refusals of the units and
of the two entry points of csrc/conv3d_hw.hip, and the restatement (tests/_hw_ref.py) in FP64 against the recording."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from densematchingbenchmark_amd import _lib
from densematchingbenchmark_amd.config import Config
from densematchingbenchmark_amd.modeling.stereo.cost_processors.aggregators import (AGGREGATORS, DeepPrunerAggregator,
                                                                                    build_cost_aggregator)
from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils import HWHourglass
from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers import FusedConv3d, conv3d_bn_relu, deconv3d_bn
from tests import _hw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "deeppruner_aggregator.npz")


def _settings(rel):
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as fp:
        return Config(json.load(fp)[rel]["settings"])


def _keys_and_shapes(module):
    sd = module.state_dict()
    return list(sd), [",".join(str(s) for s in t.shape) for t in sd.values()]


def test_state_dict_keys_and_shapes_equal_the_recording():
    z = np.load(GOLDEN)
    for tag, hip, ref in (("aggregator", DeepPrunerAggregator(R.IN_PLANES, R.HOURGLASS_IN_PLANES), R.aggregator()),
                          ("hourglass", HWHourglass(R.HOURGLASS_IN_PLANES), R.hourglass())):
        keys, shapes = [str(k) for k in z[tag + "/keys"]], [str(s) for s in z[tag + "/shapes"]]
        assert _keys_and_shapes(hip) == (keys, shapes), tag
        assert _keys_and_shapes(ref) == (keys, shapes), tag
        hip.load_state_dict(ref.state_dict(), strict=True)
    assert len(z["aggregator/keys"]) == 85
    assert {"dres0.0.0.weight", "dres2.conv1_a.0.weight", "dres2.conv3_d.1.running_var", "classify.1.weight"} <= set(z["aggregator/keys"])
    # without BatchNorm: the convolution weights only
    assert len(DeepPrunerAggregator(93, 16, batch_norm=False).state_dict()) == 15


@pytest.mark.parametrize("rel", ["configs/DeepPruner/scene_flow_4x.py", "configs/DeepPruner/scene_flow_8x.py"])
def test_aggregator_builder_on_reference_configs(rel):
    cfg = _settings(rel)
    node = cfg.model.cost_processor.cost_aggregator
    assert node.type == "DeepPruner" and node.in_planes == 93 and node.hourglass_in_planes == 16
    agg = build_cost_aggregator(cfg)
    assert type(agg) is DeepPrunerAggregator and AGGREGATORS["DeepPruner"] is DeepPrunerAggregator
    assert agg.in_planes == 93 and agg.hourglass_in_planes == 16 and agg.batch_norm == cfg.model.batch_norm
    assert isinstance(agg.dres2, HWHourglass) and agg.dres0[0][0].in_channels == 93 and agg.dres1[1][0].out_channels == 16
    assert agg.dres2.conv3_a[0].stride == (1, 2, 2) and agg.dres2.conv3_d[0].output_padding == (0, 1, 1)
    assert "cost_aggregator" in cfg.model.cost_processor and node.type == "DeepPruner"     # the node is not consumed


def test_processor_and_model_still_refuse_deeppruner():
    from densematchingbenchmark_amd.modeling import build_model
    from densematchingbenchmark_amd.modeling.stereo.cost_processors import PROCESSORS, build_cost_processor
    cfg = _settings("configs/DeepPruner/scene_flow_4x.py")
    assert set(PROCESSORS) == {'Difference', 'Concatenation', 'Correlation'}
    with pytest.raises(NotImplementedError):
        build_cost_processor(cfg)
    with pytest.raises(NotImplementedError):
        build_model(cfg, backbone=None)
    assert "AnyNet" not in AGGREGATORS     # AnyNet's aggregator stays off the registry path


def test_unit_constructor_forms():
    hw = (1, 2, 2)
    u = conv3d_bn_relu(True, 16, 32, kernel_size=3, stride=hw, padding=1, bias=False)
    assert u.stride == hw and u.hw_form and u[0].stride == hw
    u = conv3d_bn_relu(True, 32, 32, kernel_size=3, stride=(1, 1, 1), padding=1, bias=False)
    assert u.stride == 1 and not u.hw_form and u[0].stride == (1, 1, 1)
    assert conv3d_bn_relu(True, 32, 32, stride=(2, 2, 2)).stride == 2
    assert conv3d_bn_relu(True, 32, 16).hw_form and conv3d_bn_relu(True, 12, 16, stride=hw).hw_form
    d = deconv3d_bn(True, 32, 16, kernel_size=3, padding=1, output_padding=(0, 1, 1), stride=hw, bias=False)
    assert d.transposed and d.stride == hw and d.hw_form and d[0].output_padding == (0, 1, 1)
    assert not deconv3d_bn(True, 32, 32, kernel_size=3, padding=1, output_padding=(1, 1, 1), stride=(2, 2, 2)).hw_form
    for bad in (dict(stride=(2, 1, 2)), dict(stride=(2, 2, 1)), dict(stride=3), dict(stride=hw, out_planes=8),
                dict(stride=hw, out_planes=256), dict(stride=2, out_planes=16), dict(stride=(1, 2))):
        kw = dict(out_planes=32, stride=1)
        kw.update(bad)
        with pytest.raises(NotImplementedError):
            FusedConv3d(True, 16, kw["out_planes"], 3, kw["stride"], 1)
    for bad in (dict(output_padding=(1, 1, 1)), dict(output_padding=0), dict(kernel_size=4), dict(out_planes=128),
                dict(out_planes=8), dict(stride=(2, 1, 2))):
        kw = dict(out_planes=32, stride=hw, output_padding=(0, 1, 1), kernel_size=3)
        kw.update(bad)
        with pytest.raises(NotImplementedError):
            FusedConv3d(True, 64, kw["out_planes"], kw["kernel_size"], kw["stride"], 1, transposed=True, output_padding=kw["output_padding"])
    with pytest.raises(NotImplementedError, match="1, 2 or \\(1, 2, 2\\)"):
        FusedConv3d(True, 16, 32, 3, (2, 1, 2), 1)


def test_module_refusals_without_gpu():
    for c in (8, 32, 24):
        with pytest.raises(NotImplementedError, match="in_planes must be 16"):
            HWHourglass(c)
        with pytest.raises(NotImplementedError):
            DeepPrunerAggregator(93, c)
    hg = HWHourglass(16).eval()
    with torch.no_grad():
        for shape in ((1, 16, 3, 12, 16), (1, 16, 3, 16, 20), (1, 8, 3, 16, 16), (16, 3, 16, 16)):
            with pytest.raises(ValueError, match="multiples of 8"):
                hg(torch.zeros(shape))
    # inference only: training mode and inputs that carry a gradient are refused before anything is launched
    x = torch.zeros((1, 16, 2, 8, 8))
    with pytest.raises(NotImplementedError, match="no backward"):
        hg(x.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="no backward"):
        HWHourglass(16).train()(x)
    with pytest.raises(NotImplementedError, match="no backward"):
        conv3d_bn_relu(True, 32, 16).eval()(torch.zeros((1, 32, 2, 4, 4), requires_grad=True))


def _fake():
    """A non-NULL host address: the entry points must refuse before any device call, so it is never dereferenced."""
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def test_entry_points_validate_before_any_device_call():
    lib = _lib.load()
    assert lib.dmb_conv3d_k3_hw_f32(None, None, None, None, None, None, 1, 16, 32, 4, 4, 4, 2, 0, None) == 100001
    assert b"conv3d_hw" in lib.dmb_last_error()
    assert lib.dmb_deconv3d_k3_hw_f32(None, None, None, None, None, None, 1, 32, 16, 4, 4, 4, 0, None) == 100001
    keep, p = _fake()
    assert lib.dmb_conv3d_k3_hw_f32(p, p, None, None, None, p, 1, 16, 32, 0, 4, 4, 2, 0, None) == 100001
    assert lib.dmb_conv3d_k3_hw_f32(p, None, None, None, None, p, 1, 16, 32, 4, 4, 4, 2, 0, None) == 100001
    assert lib.dmb_deconv3d_k3_hw_f32(p, p, None, None, None, p, 1, 32, 16, 4, 4, -1, 0, None) == 100001
    for Co, stride_hw in ((8, 2), (256, 2), (32, 3), (32, 1), (64, 1), (128, 0), (48, 2)):
        assert lib.dmb_conv3d_k3_hw_f32(p, p, None, None, None, p, 1, 16, Co, 4, 4, 4, stride_hw, 0, None) == 100002, (Co, stride_hw)
    for Co in (8, 128, 256, 1, 48):
        assert lib.dmb_deconv3d_k3_hw_f32(p, p, None, None, None, p, 1, 32, Co, 4, 4, 4, 0, None) == 100002, Co
    assert b"deconv3d_hw" in lib.dmb_last_error()
    assert lib.dmb_abi_version() == _lib.ABI_VERSION
    del keep


def test_restatement_in_fp64_lies_on_the_recording():
    """A condition, not a tolerance: a wrong tap, skip or stride moves the output by its own magnitude, FP32 rounding by about
    1e-6 of it.  (The recording is the reference's FP32 output; the FP64 restatement is the GPU tests' yardstick.)"""
    z = np.load(GOLDEN)
    for name in list(R.GOLDEN_CASES) + list(R.HOURGLASS_CASES):
        rec = torch.from_numpy(z[name + "/out"]).double()
        f64 = R.fp64_output(name)
        assert rec.shape == f64.shape and torch.isfinite(rec).all()
        scale = f64.abs().max().item()
        err = (rec - f64).abs().max().item()
        print("%s: max|out| %.4g  max|recording - fp64| %.3g  mean %.3g" % (name, scale, err, (rec - f64).abs().mean().item()))
        assert scale > 0.1 and err <= 1e-3 * scale, (name, err, scale)
