"""DeepPruner's backbones and refinement on the CPU: keys and shapes against the real reference's recording
(tests/golden/deeppruner_features.npz, scripts/gen_golden_deeppruner_features.py), construction from the reference's two configs,
the restatement (tests/_deeppruner_features_ref.py) against the recording, the refusals of the entry point of csrc/refine_head.hip
and of the modules, and the registries that stay as they were."""
import ctypes
import inspect
import json
import os

import pytest
import torch

from densematchingbenchmark_amd import _lib, ops, ops_deeppruner
from densematchingbenchmark_amd.config import Config
from densematchingbenchmark_amd.modeling.stereo.backbones import (BACKBONES, DeepPrunerBestBackbone, DeepPrunerFastBackbone,
                                                                  PSMNetBackbone, build_backbone)
from densematchingbenchmark_amd.modeling.stereo.disp_refinement import (REFINEMENTS, DeepPrunerRefinement, RefinementHeand,
                                                                        build_disp_refinement)
from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers_2d import FusedConv2d
from tests import _deeppruner_features_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = 100001, 100002
HIP = {"best": DeepPrunerBestBackbone, "fast": DeepPrunerFastBackbone}


def _settings(rel):
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as fp:
        return Config(json.load(fp)[rel]["settings"])


def _keys_and_shapes(module):
    sd = module.state_dict()
    return list(sd), [",".join(str(s) for s in t.shape) for t in sd.values()]


def test_state_dict_keys_and_shapes_equal_the_recording():
    z = R.recording()
    for tag, hip, mine in (("refinement", DeepPrunerRefinement([74, 33], True, 2), R.refinement("r8x")),
                           ("best", DeepPrunerBestBackbone(), R.backbone("best")), ("fast", DeepPrunerFastBackbone(), R.backbone("fast"))):
        keys, shapes = [str(k) for k in z[tag + "/keys"]], [str(s) for s in z[tag + "/shapes"]]
        assert _keys_and_shapes(hip) == (keys, shapes), tag
        assert _keys_and_shapes(mine) == (keys, shapes), tag
        hip.load_state_dict(mine.state_dict(), strict=True)     # a seeded reference-style state_dict loads strictly
    assert len(z["refinement/keys"]) == 74 and len(z["best/keys"]) == 363 and len(z["fast/keys"]) == 357
    assert {"refine_blocks.0.conv.0.0.weight", "refine_blocks.1.conv.5.1.running_var", "refine_blocks.0.classify.weight",
            "refine_blocks.1.classify.weight"} <= set(str(k) for k in z["refinement/keys"])
    assert {"firstconv.0.0.weight", "layer3.0.downsample.0.bias", "branch1.1.0.weight", "lastconv.1.weight"} <= set(str(k) for k in z["best/keys"])
    assert "branch2.1.0.weight" in set(str(k) for k in z["fast/keys"]) and "branch1.1.0.weight" not in set(str(k) for k in z["fast/keys"])
    assert [str(s) for k, s in zip(z["fast/keys"], z["fast/shapes"]) if str(k) in ("layer3.0.conv1.0.weight", "layer3.0.downsample.0.weight",
                                                                                    "lastconv.0.0.weight")] == ["128,64,3,3", "128,64,1,1", "128,352,3,3"]


@pytest.mark.parametrize("rel,backbone,planes,num", [("configs/DeepPruner/scene_flow_4x.py", DeepPrunerBestBackbone, [42], 1),
                                                     ("configs/DeepPruner/scene_flow_8x.py", DeepPrunerFastBackbone, [74, 33], 2)])
def test_construction_from_the_reference_config(rel, backbone, planes, num):
    cfg = _settings(rel)
    bb, ref = build_backbone(cfg), build_disp_refinement(cfg)
    assert type(bb) is backbone and BACKBONES[cfg.model.backbone.type] is backbone and bb.batch_norm is True
    assert type(ref) is DeepPrunerRefinement and REFINEMENTS["DeepPruner"] is DeepPrunerRefinement
    assert (list(ref.in_planes_list), ref.num, ref.batch_norm) == (planes, num, True) and len(ref.refine_blocks) == num
    assert "backbone" in cfg.model and "disp_refinement" in cfg.model                      # the nodes are not consumed
    for blk, ci in zip(ref.refine_blocks, planes):
        assert type(blk) is RefinementHeand and blk.in_planes == ci
        assert [(u.in_planes, u.out_planes, u.dilation, u.has_bn, u.has_relu, u[0].bias is None) for u in blk.conv] == [
            (ci, 32, 1, True, True, True), (32, 32, 1, True, True, True), (32, 32, 1, True, True, True), (32, 16, 2, True, True, True),
            (16, 16, 4, True, True, True), (16, 16, 1, True, True, True)]
        assert all(type(u) is FusedConv2d for u in blk.conv)
        assert isinstance(blk.classify, torch.nn.Conv2d) and blk.classify.weight.shape == (1, 16, 3, 3) and blk.classify.bias is None
    assert isinstance(bb, PSMNetBackbone) == (backbone is DeepPrunerBestBackbone)          # Best alone is that network
    if backbone is DeepPrunerFastBackbone:
        assert not hasattr(bb, "_features") and not hasattr(bb, "_forward_train")
        first = bb.layer3[0]
        assert first.conv1.split_halves and first.downsample.split_halves and first.conv1.stride == first.downsample.stride == 2
        assert not first.conv2.split_halves and not any(m.split_halves for m in bb.layer2.modules() if isinstance(m, FusedConv2d))
        assert not hasattr(bb, "branch1") and bb.lastconv[0].in_planes == 352 and bb.layer4[0].conv1.dilation == 1
    else:
        assert bb.lastconv[0].in_planes == 320 and bb.layer4[0].conv1.dilation == 2 and bb.branch1[0].kernel_size == (64, 64)
        assert not any(m.split_halves for m in bb.modules() if isinstance(m, FusedConv2d))
    with pytest.raises(NotImplementedError):
        build_disp_refinement(Config(dict(model=dict(batch_norm=True, disp_refinement=dict(type="AnyNet", in_planes=3)))))


def _check_on_recording(got, rec, what):
    """A condition, not a tolerance (test_recording_lies_on_the_fp64_restatement of the processor): a wrong tap, key or stage moves
    an output by its own magnitude, FP32 rounding by about 1e-5 of it at most."""
    rec = torch.from_numpy(rec).double()
    assert rec.shape == got.shape and torch.isfinite(rec).all(), (what, rec.shape, got.shape)
    scale, err = got.abs().max().item(), (rec - got.double()).abs().max().item()
    print("%s: max|out| %.4g  max|recording - restatement| %.3g" % (what, scale, err))
    assert scale > 0.1 and err <= 1e-3 * scale, (what, err, scale)


@pytest.mark.parametrize("name", list(R.REFINE_CASES))
def test_refinement_restatement_reproduces_the_recording(name):
    z = R.recording()
    (planes, num, B, (H, W)), _ = R.REFINE_CASES[name]
    for i, (refined, up) in enumerate(R.fp64_refinement(name)):
        _check_on_recording(refined, z["%s/refined%d" % (name, i)], "%s refined%d" % (name, i))
        _check_on_recording(up, z["%s/up%d" % (name, i)], "%s up%d" % (name, i))
        assert up.shape == (B, 1, (H << i) * 2, (W << i) * 2)
        clamped = (torch.from_numpy(z["%s/refined%d" % (name, i)]) == 0).float().mean().item()
        assert 0.05 <= clamped <= 0.95, (name, i, clamped)            # the ReLU takes both branches


@pytest.mark.parametrize("name", list(R.BACKBONE_CASES))
def test_backbone_restatement_reproduces_the_recording(name):
    z = R.recording()
    _, (B, _, H, W), _, strides = R.BACKBONE_CASES[name]
    want = [[B, 32, H // 4, W // 4], [B, 32, H // 2, W // 2]] if name == "best" else \
        [[B, 32, H // 8, W // 8], [B, 64, H // 4, W // 4], [B, 32, H // 2, W // 2]]
    assert z[name + "/full_shapes"].tolist() == want
    x = R.backbone_input(name)
    with torch.no_grad():
        maps = R.flatten(R.backbone(name)._forward(x))                # FP32 on the CPU
    assert [list(m.shape) for m in maps] == want
    for i, sub in enumerate(R.subsample(name, maps)):
        _check_on_recording(sub, z["%s/map%d" % (name, i)], "%s map%d" % (name, i))


def _fake():
    """A non-NULL host address: the entry point must refuse before any device call, so it is never dereferenced."""
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def test_entry_point_validates_before_any_device_call():
    lib = _lib.load()
    keep, p = _fake()
    head = lib.dmb_refine_head_up2_f32
    for args, code in (((None, None, None, None, 1, 16, 8, 8), EINVAL), ((None, p, p, p, 1, 16, 8, 8), EINVAL),
                       ((p, None, p, p, 1, 16, 8, 8), EINVAL), ((p, p, None, p, 1, 16, 8, 8), EINVAL), ((p, p, p, None, 1, 16, 8, 8), EINVAL),
                       ((p, p, p, p, 0, 16, 8, 8), EINVAL), ((p, p, p, p, 1, 16, 0, 8), EINVAL), ((p, p, p, p, 1, 16, 8, -2), EINVAL),
                       ((p, p, p, p, 1, 0, 8, 8), EUNSUPPORTED), ((p, p, p, p, 1, 17, 8, 8), EUNSUPPORTED),
                       ((p, p, p, p, 1, -1, 8, 8), EUNSUPPORTED), ((p, p, p, p, 1, 16, 1 << 13, 1 << 13), EUNSUPPORTED),   # 4 GiB item
                       ((p, p, p, p, 1, 1, 1 << 14, 1 << 13), EUNSUPPORTED)):                                              # a 2 GiB output
        assert head(*args, None) == code, args
        assert b"refine_head" in lib.dmb_last_error(), args
    assert lib.dmb_abi_version() == _lib.ABI_VERSION
    del keep


def test_what_must_not_change():
    from densematchingbenchmark_amd.modeling import build_model
    from densematchingbenchmark_amd.modeling.stereo.cost_processors import PROCESSORS, build_cost_processor
    from densematchingbenchmark_amd.modeling.stereo.models import _META_ARCHITECTURES
    for rel in ("configs/DeepPruner/scene_flow_4x.py", "configs/DeepPruner/scene_flow_8x.py"):
        cfg = _settings(rel)
        with pytest.raises(NotImplementedError):
            build_cost_processor(cfg)
        with pytest.raises(NotImplementedError):
            build_model(cfg, backbone=None)
        with pytest.raises(NotImplementedError):
            build_model(cfg)
    assert set(PROCESSORS) == {'Difference', 'Concatenation', 'Correlation'}
    assert set(_META_ARCHITECTURES) == {"GeneralizedStereoModel", "AnyNet"}
    # the new launching wrapper lives next to ops, not in it, and allocates through the module's own ``torch``
    assert not hasattr(ops, "refine_head_up2") and ops_deeppruner.torch is torch
    src = inspect.getsource(ops_deeppruner.refine_head_up2)
    assert 'launch("dmb_' in src and "torch.empty(" in src and "empty_like" not in src and "new_empty" not in src
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES) and "dmb_refine_head_up2_f32" in _lib.SIGNATURES
    # FusedConv2d gained exactly one form
    for bad in ((3, 2, 1, 96), (3, 2, 1, 127), (3, 2, 2, 128), (5, 2, 1, 128), (3, 2, 1, 129)):
        k, s, d, co = bad
        with pytest.raises(NotImplementedError):
            FusedConv2d(True, 64, co, k, s, d * (k // 2), d)
    assert FusedConv2d(True, 64, 128, 3, 2, 1, 1).split_halves and FusedConv2d(True, 64, 128, 1, 2, 0, 1).split_halves
    assert not FusedConv2d(True, 64, 128, 3, 1, 1, 1).split_halves and not FusedConv2d(True, 64, 64, 3, 2, 1, 1).split_halves


def test_wrapper_refuses_bad_operands_on_the_host():
    x, w, init = torch.zeros((2, 5, 4, 6)), torch.zeros((1, 5, 3, 3)), torch.zeros((2, 1, 4, 6))
    for args in ((x[0], w, init), (x, w[0], init), (x, torch.zeros((1, 4, 3, 3)), init), (x, torch.zeros((2, 5, 3, 3)), init),
                 (torch.zeros((2, 17, 4, 6)), torch.zeros((1, 17, 3, 3)), init), (x.double(), w, init), (x, w.double(), init),
                 (x, w, init.double()), (x, w, torch.zeros((2, 1, 4, 5))), (x, w, torch.zeros((1, 1, 4, 6))), (x, w, torch.zeros((2, 2, 4, 6)))):
        with pytest.raises(_lib.DmbLibraryError):
            ops_deeppruner.refine_head_up2(*args)


def test_training_and_gradients_are_refused():
    disps, fms = R.refine_inputs("rodd")
    ref = DeepPrunerRefinement([7], True, 1).eval()
    with pytest.raises(NotImplementedError, match="no backward"):
        ref(list(disps), fms)                                       # eval(), but grad mode on and the parameters require grad
    with pytest.raises(NotImplementedError, match="no backward"):
        with torch.no_grad():
            ref.train()(list(disps), fms)
    ref.eval().requires_grad_(False)
    with pytest.raises(NotImplementedError, match="no backward"):
        ref([disps[0].clone().requires_grad_()], fms)
    with pytest.raises(NotImplementedError, match="no backward"):
        ref(list(disps), [fms[0].clone().requires_grad_()])
    head = ref.refine_blocks[0]
    guide = torch.zeros((2, 7, 5, 13))
    with pytest.raises(NotImplementedError, match="no backward"):
        head(disps[0], guide.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="no backward"):
        head.classify(torch.zeros((2, 16, 5, 13)), disps[0].clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="no backward"):
        head.train()(disps[0], guide)
    img = torch.zeros((1, 3, 64, 64))
    for cls in (DeepPrunerBestBackbone, DeepPrunerFastBackbone):
        bb = cls().eval()
        with pytest.raises(NotImplementedError, match="no backward"):
            bb(img, img)                                            # its own parameters require gradients
        with pytest.raises(NotImplementedError, match="no backward"):
            with torch.no_grad():
                bb.train()(img, img)
        bb.eval().requires_grad_(False)
        with pytest.raises(NotImplementedError, match="no backward"):
            bb(img, img.clone().requires_grad_())
        with pytest.raises(ValueError):
            bb(img)
    unit = FusedConv2d(True, 64, 128, 3, 2, 1, 1).eval()
    with pytest.raises(NotImplementedError, match="no backward"):
        unit(torch.zeros((1, 64, 8, 8)))


def test_two_view_forward_splits_nested_outputs_of_one_batch():
    """The one-batch path (CPU tensors, or ``ops.set_view_streams(False)``): both views go through ``fn`` as one batch of 2B and
    every tensor of a nested result is cut into its two halves, the containers keeping their types; a bare tensor as before."""
    left, right = torch.arange(6.0).view(3, 2), torch.arange(6.0, 12.0).view(3, 2)
    calls = []

    def fn(x):
        calls.append(tuple(x.shape))
        return x * 2, [x + 1, (x - 1,)]

    (fl, fr) = ops.two_view_forward(fn, left, right)
    assert calls == [(6, 2)]
    for got, src in ((fl, left), (fr, right)):
        assert isinstance(got, tuple) and isinstance(got[1], list) and isinstance(got[1][1], tuple)
        assert torch.equal(got[0], src * 2) and torch.equal(got[1][0], src + 1) and torch.equal(got[1][1][0], src - 1)
    bl, br = ops.two_view_forward(lambda x: x * 3, left, right)
    assert torch.equal(bl, left * 3) and torch.equal(br, right * 3)
