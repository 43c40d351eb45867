"""AnyNet on the CPU: the functional restatement (tests/_anynet_ref.py) against the real reference's recorded forward
(tests/golden/anynet.npz, scripts/gen_golden_anynet.py), the config and state_dict boundary, and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

from densematchingbenchmark_amd.config import Config
from tests import _anynet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "anynet.npz")


def _golden():
    return np.load(GOLDEN)


def golden_state(dtype=torch.float32):
    z = _golden()
    sd = {k[2:]: torch.from_numpy(z[k]).to(dtype) for k in z.files if k.startswith("w/")}
    for name, dt in zip(z["sd_names"], z["sd_dtypes"]):
        if dt == "int64":
            sd[str(name)] = torch.zeros((), dtype=torch.int64)
    return sd


def _cfg():
    return Config.fromfile(os.path.join(ROOT, "configs", "AnyNet", "scene_flow.py"))


def _ref_settings():
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as fp:
        return Config(json.load(fp)["configs/AnyNet/scene_flow.py"]["settings"])


def test_restatement_matches_reference_recording():
    """FP32: the same torch ops in the same order as the reference -- bit-exact at 8 threads; FP64 to rounding."""
    z = _golden()
    cfg = _cfg().model.cost_processor
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            trace = {}
            left, right = R.golden_inputs(dtype=dtype)
            with torch.no_grad():
                disps, costs = R.forward(left, right, golden_state(dtype), cfg, trace=trace)
            got = {"cost_init": trace["cost_init"], "cost_w8": trace["cost_w8"], "cost_w4": trace["cost_w4"],
                   "disp_init": trace["disp_init"], "res_w8": trace["res_w8"], "res_w4": trace["res_w4"],
                   "disp_w8": trace["disp_w8"], "disp_w4": trace["disp_w4"], "refined": trace["refined"]}
            for i, s in enumerate((16, 8, 4)):
                got["fms_left_%d" % s], got["fms_right_%d" % s] = trace["fms_left"][i], trace["fms_right"][i]
            if tag == "f32":
                got["disps"] = torch.stack(disps[:4])
                for i in range(1, 4):
                    assert torch.equal(disps[3 + i], disps[i - 1] - disps[i])
            for k, v in got.items():
                ref = z["%s/%s" % (tag, k)]
                if tag == "f32":
                    assert np.array_equal(v.numpy(), ref), k
                else:
                    assert np.abs(v.numpy() - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), k
            assert [c.shape for c in costs] == [trace["cost_w4"].shape, trace["cost_w8"].shape, trace["cost_init"].shape]
    finally:
        torch.set_num_threads(threads)


def test_configs_build_and_reference_state_dict_loads_strictly():
    from densematchingbenchmark_amd.modeling import build_model
    z = _golden()
    shapes = {str(n): tuple(int(s) for s in str(sh).split(",") if s) for n, sh in zip(z["sd_names"], z["sd_shapes"])}
    for cfg in (_cfg(), _ref_settings()):
        model = build_model(cfg)
        assert type(model).__name__ == "AnyNet"
        ours = model.state_dict()
        assert set(ours) == set(shapes)
        assert all(tuple(v.shape) == shapes[k] for k, v in ours.items())
        model.load_state_dict(golden_state(), strict=True)
        assert 46000 < sum(p.numel() for p in model.parameters()) < 48000        # "47 K parameters" (ResultOfAnyNet.md)


def test_refusals():
    from densematchingbenchmark_amd.modeling import build_model
    from densematchingbenchmark_amd.modeling.stereo.layers import bn_relu_conv, bn_relu_conv3d
    from densematchingbenchmark_amd.modeling.stereo.layers.preact import PreActConv, SmallConvBnRelu
    cfg = _cfg()
    with pytest.raises(NotImplementedError, match="cost-path-alone"):
        build_model(cfg, backbone=None)
    with pytest.raises(NotImplementedError, match="cost-path-alone"):
        build_model(_ref_settings(), backbone=None)
    model = build_model(cfg)
    batch = dict(leftImage=torch.zeros(1, 3, 64, 128), rightImage=torch.zeros(1, 3, 64, 128))
    with pytest.raises(NotImplementedError, match="inference only"):
        model.train()(batch)
    model.eval()
    with pytest.raises(NotImplementedError, match="no backward"):
        model(batch)                                        # parameters require gradients and grad mode is on
    unit = bn_relu_conv(True, 4, 8).eval()
    with pytest.raises(NotImplementedError, match="no backward"):
        unit(torch.zeros(1, 4, 8, 8))                       # its own parameters require gradients
    unit.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="no backward"):
        unit(torch.zeros(1, 4, 8, 8, requires_grad=True))   # the input does
    with pytest.raises(NotImplementedError, match="inference only"):
        unit.train()(torch.zeros(1, 4, 8, 8))
    for make in (lambda: bn_relu_conv(True, 65, 8), lambda: bn_relu_conv3d(True, 16, 33), lambda: SmallConvBnRelu(True, 3, 48),
                 lambda: bn_relu_conv3d(True, 4, 4, stride=2), lambda: bn_relu_conv(True, 4, 4, kernel_size=5, padding=2)):
        with pytest.raises(NotImplementedError):
            make()
    with pytest.raises(NotImplementedError, match="track_running_stats"):
        PreActConv(True, 4, 4, ndim=2, bn_kwargs=dict(track_running_stats=False))
    # DeepPruner and the registries stay as they were
    from densematchingbenchmark_amd.modeling.stereo.cost_processors import PROCESSORS, build_cost_processor
    assert set(PROCESSORS) == {'Difference', 'Concatenation', 'Correlation'}
    with pytest.raises(NotImplementedError):
        build_cost_processor(cfg)
