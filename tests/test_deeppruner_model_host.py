"""The DeepPruner model on the CPU: reached by import, built from the reference's two configs and from this repository's two config
files, keys and shapes against the real reference's recording (tests/golden/deeppruner_model.npz,
scripts/gen_golden_deeppruner_model.py), the registries that stay as they were, every refusal of the model before a launch, the
restatement (tests/_deeppruner_model_ref.py) against the recording, the refusals of the entry point of
csrc/deeppruner_final_maps.hip and of its wrapper, and ``init_model``'s dispatch."""
import ctypes
import inspect
import json
import os

import pytest
import torch

from densematchingbenchmark_amd import _lib, ops, ops_deeppruner
from densematchingbenchmark_amd.config import Config
from tests import _deeppruner_model_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = 100001, 100002
RELS = {name: case[0] for name, case in R.CASES.items()}


def _reference_settings(rel):
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as fp:
        return json.load(fp)[rel]["settings"]


def _plain(node):
    if isinstance(node, dict):
        return {k: _plain(v) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return [_plain(v) for v in node]
    return node


def _model(name, source="file"):
    from densematchingbenchmark_amd.modeling.stereo.models import DeepPruner       # fails on the parent commit
    cfg = Config.fromfile(os.path.join(ROOT, RELS[name])) if source == "file" else Config(_reference_settings(RELS[name]))
    return DeepPruner(cfg)


@pytest.mark.parametrize("name", list(R.CASES))
def test_import_construction_and_state_dict(name):
    from densematchingbenchmark_amd.modeling.stereo.backbones import DeepPrunerBestBackbone, DeepPrunerFastBackbone
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.DeepPruner import DeepPrunerProcessor
    from densematchingbenchmark_amd.modeling.stereo.disp_refinement import DeepPrunerRefinement
    from densematchingbenchmark_amd.modeling.stereo.disp_samplers import DeepPrunerSampler
    z = R.recording()
    keys, shapes = [str(k) for k in z[name + "/keys"]], [str(s) for s in z[name + "/shapes"]]
    assert len(keys) == {"4x": 363 + 258 + 37, "8x": 357 + 258 + 74}[name]
    file_cfg = Config.fromfile(os.path.join(ROOT, RELS[name]))
    assert _plain(file_cfg.model) == _plain(_reference_settings(RELS[name])["model"])    # the new config's model node is the reference's
    mine = R.model(name)
    for source in ("file", "reference"):
        m = _model(name, source)
        sd = m.state_dict()
        assert (list(sd), [",".join(str(s) for s in t.shape) for t in sd.values()]) == (keys, shapes), (name, source)
        assert type(m.backbone) is {"4x": DeepPrunerBestBackbone, "8x": DeepPrunerFastBackbone}[name]
        assert type(m.disp_sampler) is DeepPrunerSampler and type(m.cost_processor) is DeepPrunerProcessor
        assert type(m.disp_refinement) is DeepPrunerRefinement and m.down_sample == {"4x": 4, "8x": 8}[name]
        assert not [k for k, _ in m.named_parameters(recurse=False)] and not list(m.disp_sampler.parameters())
        assert m.disp_sampler.max_disp == {"4x": 48, "8x": 24}[name] and m.max_disp == 192
        m.load_state_dict(mine.state_dict(), strict=True)          # the restatement's seeded, reference-style state loads strictly
    assert list(mine.state_dict()) == keys


def test_registries_stay_as_they_were():
    from densematchingbenchmark_amd.modeling import build_model
    from densematchingbenchmark_amd.modeling.stereo import models
    from densematchingbenchmark_amd.modeling.stereo.cost_processors import PROCESSORS, build_cost_processor
    for name in R.CASES:
        for cfg in (Config(_reference_settings(RELS[name])), Config.fromfile(os.path.join(ROOT, RELS[name]))):
            with pytest.raises(NotImplementedError):
                build_cost_processor(cfg)
            with pytest.raises(NotImplementedError):
                build_model(cfg)
            with pytest.raises(NotImplementedError):
                build_model(cfg, backbone=None)
    assert set(PROCESSORS) == {'Difference', 'Concatenation', 'Correlation'}
    assert set(models._META_ARCHITECTURES) == {"GeneralizedStereoModel", "AnyNet"}
    assert models.DeepPruner.__name__ == "DeepPruner" and models.DeepPruner not in models._META_ARCHITECTURES.values()
    # the new launching wrapper lives next to ops, not in it, and allocates through the module's own ``torch``
    assert not hasattr(ops, "deeppruner_final_maps") and ops_deeppruner.torch is torch
    src = inspect.getsource(ops_deeppruner.deeppruner_final_maps)
    assert 'launch("dmb_' in src and "torch.empty(" in src and "empty_like" not in src and "new_empty" not in src
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES) and "dmb_deeppruner_final_maps_f32" in _lib.SIGNATURES
    assert _lib.load().dmb_abi_version() == _lib.ABI_VERSION


def test_refusals_come_before_any_launch(monkeypatch):
    """Every launch goes through ``_lib.load()``: with it replaced by a function that fails the test, a refusal that raises its
    own error has launched nothing."""
    from densematchingbenchmark_amd.modeling.stereo.models import DeepPruner
    cfg = Config.fromfile(os.path.join(ROOT, RELS["4x"]))
    for bad in (None, "torch", "none", 1):
        with pytest.raises(NotImplementedError, match="backbone"):
            DeepPruner(cfg, backbone=bad)
    for ok in ("auto", "hip"):
        DeepPruner(cfg, backbone=ok)
    other = Config.fromfile(os.path.join(ROOT, RELS["4x"]))
    other.model.meta_architecture = "GeneralizedStereoModel"
    with pytest.raises(NotImplementedError, match="meta_architecture"):
        DeepPruner(other)

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_launch)
    img = torch.zeros((1, 3, 256, 288))
    for name, bad_hw in (("4x", (258, 264)), ("4x", (256, 290)), ("4x", (256, 264)), ("8x", (256, 288)), ("8x", (260, 320))):
        m = _model(name).eval().requires_grad_(False)
        with pytest.raises(ValueError, match="multiples of"):
            m(dict(leftImage=torch.zeros((1, 3) + bad_hw), rightImage=torch.zeros((1, 3) + bad_hw)))
    m = _model("4x").eval()
    batch = dict(leftImage=img, rightImage=img)
    with pytest.raises(NotImplementedError, match="no backward"):
        m(batch)                                                        # eval(), grad mode on, the parameters require gradients
    with pytest.raises(NotImplementedError, match="no backward"):
        with torch.no_grad():
            m.train()(batch)
    m.eval().requires_grad_(False)
    for key in ("leftImage", "rightImage"):
        with pytest.raises(NotImplementedError, match="no backward"):
            m(dict(batch, **{key: img.clone().requires_grad_()}))
    with pytest.raises(NotImplementedError, match="no backward"):
        m(dict(batch, patchMatchNoise=torch.zeros((1, 12, 64, 72)).requires_grad_()))
    for noise in (torch.zeros((1, 12, 64, 71)), torch.zeros((1, 14, 64, 72)), torch.zeros((2, 12, 64, 72)), torch.zeros((12, 64, 72)),
                  torch.zeros((1, 12, 64, 72), dtype=torch.float64), torch.zeros((1, 12, 64, 72), device="meta"), "noise"):
        with pytest.raises(ValueError, match="patchMatchNoise"):
            m(dict(batch, patchMatchNoise=noise))
    with pytest.raises(ValueError, match="one shape"):
        m(dict(leftImage=img, rightImage=torch.zeros((1, 3, 256, 320))))


def test_cpu_tensors_meet_the_no_cpu_fallback_error():
    m = _model("4x").eval().requires_grad_(False)
    img = torch.zeros((1, 3, 256, 288))
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        m(dict(leftImage=img, rightImage=img, patchMatchNoise=torch.zeros((1, 12, 64, 72))))
    d = torch.zeros((1, 1, 4, 4))
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        ops_deeppruner.deeppruner_final_maps([d], d, d, (8, 8))


def _check_on_recording(got, rec, what):
    """A condition, not a tolerance (tests/test_deeppruner_features_host.py): a wrong tap, key or stage moves an output by its own
    magnitude everywhere.  FP32 rounding, amplified by PatchMatch's softmax, moves it by about 1e-3 of it at most
    (scripts/gen_golden_deeppruner_model.py prints the reference's distance from the FP64 yardstick), and on another CPU than the
    recording's a few ``target > 0`` decisions at T ~ 0 fall the other way and move the pixels around them by up to 1e-2 of it
    (tests/_deeppruner_model_ref.py): so the mean and the 99th percentile are held, not the maximum.  On the recording's CPU and
    thread count the restatement equals the recording bit for bit, which the generator asserts."""
    rec = torch.from_numpy(rec)
    assert rec.shape == got.shape and torch.isfinite(rec).all(), (what, rec.shape, got.shape)
    d = (rec.double() - got.double()).abs().flatten()
    scale, mean, q99 = got.abs().max().item(), d.mean().item(), torch.quantile(d, 0.99).item()
    print("%s: max|out| %.4g  |recording - restatement|: mean %.3g  99th percentile %.3g  max %.3g" % (what, scale, mean, q99, d.max()))
    assert scale > 0.1 and mean <= 1e-3 * scale and q99 <= 5e-3 * scale, (what, mean, q99, scale)


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_reproduces_the_recording(name):
    z = R.recording()
    _, _, _, planes, (B, _, H, W), _, _ = R.CASES[name]
    K, s = len(planes) + 1, 2 << len(planes)
    out = R.fp32_outputs(name)
    assert len(out["disps"]) == K + 4 and z[name + "/full_shapes"].tolist() == [[B, 1, H, W]] * (K + 4)
    for i, sub in enumerate(R.subsample(name, out["disps"])):
        _check_on_recording(sub, z["%s/disp%d" % (name, i)], "%s disp%d" % (name, i))
    for key in ("min_disparity", "max_disparity"):
        assert out[key].shape == (B, 1, H // s, W // s)
        _check_on_recording(out[key], z["%s/%s" % (name, key)], "%s %s" % (name, key))
    # what the recording was asserted to be when it was written: an ordered range, both branches of every ReLU, live residuals, and
    # a second scaling of the range maps that shows
    lo, hi = torch.from_numpy(z[name + "/min_disparity"]), torch.from_numpy(z[name + "/max_disparity"])
    assert (lo < hi).float().mean() >= 0.6
    for i in range(K - 1):
        zeros = (torch.from_numpy(z["%s/disp%d" % (name, i)]) == 0).float().mean().item()
        assert 0.005 <= zeros <= 0.995, (name, i, zeros)
    assert all(z["%s/disp%d" % (name, i)].max() > 0 for i in (K + 2, K + 3))
    Mn = R.subsample(name, [R.up(lo, (H, W))])[0]
    assert int((torch.from_numpy(z["%s/disp%d" % (name, K)]) != Mn).sum()) >= 1


def test_tail_restatement_rounds_as_the_reference_does():
    """(d * W) / w is two roundings per tap, and the full-size range maps are scaled a second time."""
    g = torch.Generator().manual_seed(7)
    d = torch.rand((1, 1, 6, 60), generator=g) * 50
    assert not torch.equal((d * 240) / 60, d * 4) and not torch.equal((d * 240) / 240, d)
    lo, hi = torch.rand((1, 1, 3, 30), generator=g) * 20, torch.rand((1, 1, 3, 30), generator=g) * 20 + 20
    maps = R.final_maps([d * 2, d[:, :, ::1, ::2].contiguous()], lo, hi, (12, 240))
    assert len(maps) == 6 and all(m.shape == (1, 1, 12, 240) for m in maps)
    Mn, D = R.up(lo, (12, 240)), R.up(d[:, :, ::1, ::2].contiguous(), (12, 240))
    assert torch.equal(maps[1], D) and torch.equal(maps[2], (Mn * 240) / 240) and not torch.equal(maps[2], Mn)
    assert torch.equal(maps[4], (D - Mn).abs())


def _fake():
    """A non-NULL host address: the entry point must refuse before any device call, so it is never dereferenced."""
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def test_entry_point_validates_before_any_device_call():
    lib = _lib.load()
    keep, p = _fake()
    hs, ws = _lib.host_ints([8, 4, 2]), _lib.host_ints([8, 4, 2])
    fn = lib.dmb_deeppruner_final_maps_f32
    ok = (p, p, p, hs, ws, p, p, p, 3, 1, 2, 2, 8, 8)

    def call(**change):
        names = ("d0", "d1", "d2", "hs", "ws", "lo", "hi", "out", "K", "B", "h", "w", "H", "W")
        args = dict(zip(names, ok))
        args.update(change)
        return fn(*[args[n] for n in names], None)

    big = _lib.host_ints([1 << 15, 4, 2])
    for change, code in ((dict(d0=None), EINVAL), (dict(d1=None), EINVAL), (dict(d2=None), EINVAL), (dict(hs=None), EINVAL),
                         (dict(ws=None), EINVAL), (dict(lo=None), EINVAL), (dict(hi=None), EINVAL), (dict(out=None), EINVAL),
                         (dict(B=0), EINVAL), (dict(h=0), EINVAL), (dict(w=-1), EINVAL), (dict(H=0), EINVAL), (dict(W=-8), EINVAL),
                         (dict(hs=_lib.host_ints([8, 0, 2])), EINVAL), (dict(ws=_lib.host_ints([8, 4, -2])), EINVAL),
                         (dict(K=0), EUNSUPPORTED), (dict(K=4), EUNSUPPORTED), (dict(K=-1), EUNSUPPORTED),
                         (dict(H=1 << 15, W=1 << 14), EUNSUPPORTED),                   # a 2 GiB output item
                         (dict(h=1 << 15, w=1 << 14), EUNSUPPORTED),                   # a 2 GiB range map
                         (dict(hs=big, ws=_lib.host_ints([1 << 14, 4, 2])), EUNSUPPORTED),   # a 2 GiB list map
                         (dict(B=65536), EUNSUPPORTED), (dict(H=1 << 19, W=1), EUNSUPPORTED)):   # beyond the grid
        assert call(**change) == code, change
        assert b"deeppruner_final_maps" in lib.dmb_last_error(), change
    assert call(K=2, d1=None) == EINVAL and call(K=1, d0=None) == EINVAL       # a NULL among the K maps the list holds
    assert lib.dmb_abi_version() == _lib.ABI_VERSION
    del keep


def test_wrapper_refuses_bad_operands_on_the_host():
    d, lo = torch.zeros((2, 1, 8, 8)), torch.zeros((2, 1, 2, 2))
    for args in (([], lo, lo, (8, 8)), ([d] * 4, lo, lo, (8, 8)), ([d.double()], lo, lo, (8, 8)), ([d], lo.double(), lo, (8, 8)),
                 ([d], lo, lo.double(), (8, 8)), ([d], lo, torch.zeros((2, 1, 2, 3)), (8, 8)), ([d[0]], lo, lo, (8, 8)),
                 ([d, torch.zeros((1, 1, 4, 4))], lo, lo, (8, 8)), ([torch.zeros((2, 2, 8, 8))], lo, lo, (8, 8)),
                 ([d], torch.zeros((1, 1, 2, 2)), torch.zeros((1, 1, 2, 2)), (8, 8)), ([d], lo, lo, (0, 8)), ([d], lo, lo, (8, -1))):
        with pytest.raises(_lib.DmbLibraryError):
            ops_deeppruner.deeppruner_final_maps(*args)


def test_init_model_dispatches_by_import(tmp_path):
    from densematchingbenchmark_amd.apis import init_model
    from densematchingbenchmark_amd.modeling.stereo.models import DeepPruner, GeneralizedStereoModel
    for name in R.CASES:
        m = init_model(os.path.join(ROOT, RELS[name]), None, "cpu")
        assert type(m) is DeepPruner and not m.training and m.cfg.model.meta_architecture == "DeepPruner"
        assert next(m.parameters()).device.type == "cpu"
    state = R.model("4x").state_dict()
    m = init_model(Config.fromfile(os.path.join(ROOT, RELS["4x"])), {"state_dict": {"module." + k: v for k, v in state.items()}}, "cpu")
    assert torch.equal(m.state_dict()["disp_refinement.refine_blocks.0.classify.weight"],
                       state["disp_refinement.refine_blocks.0.classify.weight"])
    with pytest.raises(RuntimeError):
        init_model(os.path.join(ROOT, RELS["8x"]), {"state_dict": state}, "cpu")       # the 4x keys do not fit the 8x model
    psm = init_model(os.path.join(ROOT, "configs", "PSMNet", "scene_flow.py"), None, "cpu")
    assert type(psm) is GeneralizedStereoModel and not psm.training
