"""DeepPruner's disparity sampler on the CPU: the functional restatement (tests/_deeppruner_ref.py) against the real reference's
recorded outputs (tests/golden/deeppruner_sampler.npz, scripts/gen_golden_deeppruner_sampler.py), the builder, the refusals."""
import json
import os

import numpy as np
import pytest
import torch

from densematchingbenchmark_amd import _lib
from densematchingbenchmark_amd.config import Config
from densematchingbenchmark_amd.modeling.registry import UnknownType
from densematchingbenchmark_amd.modeling.stereo.disp_samplers import (SAMPLER, DeepPrunerSampler, PatchMatch, UniformSampler,
                                                                      build_disp_sampler)
from tests import _deeppruner_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "deeppruner_sampler.npz")


def _settings(rel):
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as fp:
        return Config(json.load(fp)[rel]["settings"])


def test_restatement_matches_reference_recording():
    """FP32 at 8 threads: the same torch operations in the same order as the reference -- bit for bit, both stages."""
    z = np.load(GOLDEN)
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        for name, (shape, max_disp, _, seed) in R.GOLDEN_CASES.items():
            assert int(z[name + "/seed"]) == seed
            left, right, noise, lo, hi = R.golden_inputs(name)
            with torch.no_grad():
                pre = R.sampler('pre', left, right, noise=noise, max_disp=max_disp)
                post = R.sampler('post', left, right, lo, hi, max_disp=max_disp)
            assert torch.equal(pre, torch.from_numpy(z[name + "/pre"])), name
            assert torch.equal(post, torch.from_numpy(z[name + "/post"])), name
            # the FP64 evaluation is the yardstick of the GPU tests: the recording lies within 1e-4 of it
            with torch.no_grad():
                f64 = R.sampler('pre', left.double(), right.double(), noise=noise.double(), max_disp=max_disp)
            assert (pre.double() - f64).abs().max().item() <= 1e-4
    finally:
        torch.set_num_threads(threads)


def test_recorded_reference_output_structure():
    """What the GPU tests require of the HIP result holds for the reference's own output: the ends are the range, every inner
    sample lies in its interval, the channels do not decrease."""
    z = np.load(GOLDEN)
    for name, (shape, max_disp, _, _) in R.GOLDEN_CASES.items():
        pre = torch.from_numpy(z[name + "/pre"])
        P = pre.shape[1] - 2
        assert (pre[:, 0] == 0).all() and (pre[:, -1] == max_disp).all()
        for p in range(P):
            assert (pre[:, 1 + p] >= max_disp * (p + 1) / (P + 1) - 1e-4).all()
            assert (pre[:, 1 + p] <= max_disp * (p + 2) / (P + 1) + 1e-4).all()
        assert (pre[:, 1:] >= pre[:, :-1]).all()


@pytest.mark.parametrize("rel,max_disp", [("configs/DeepPruner/scene_flow_4x.py", 48), ("configs/DeepPruner/scene_flow_8x.py", 24)])
def test_builder_on_reference_configs(rel, max_disp):
    cfg = _settings(rel)
    s = build_disp_sampler(cfg)
    assert type(s) is DeepPrunerSampler and SAMPLER["DeepPruner"] is DeepPrunerSampler
    assert s.max_disp == max_disp and s.batch_norm == cfg.model.batch_norm
    assert s.patch_match_disparity_sample_number == 14 and s.uniform_disparity_sample_number == 9
    assert s.iterations == 3 and s.temperature == 7 and s.propagation_filter_size == 3
    assert isinstance(s.patch_match, PatchMatch) and isinstance(s.uniform_sampler, UniformSampler)
    assert s.patch_match.disparity_sample_number == 14 and s.patch_match.iterations == 3 and s.patch_match.temperature == 7
    assert s.uniform_sampler.disparity_sample_number == 9 and s.disparity_sample_range.max_disp == max_disp
    assert list(s.parameters()) == [] and list(s.buffers()) == [] and len(s.state_dict()) == 0
    assert "disp_sampler" in cfg.model and cfg.model.disp_sampler.type == "DeepPruner"     # the node is not consumed


def test_builder_refusals():
    cfg = _settings("configs/DeepPruner/scene_flow_4x.py")
    cfg.model.disp_sampler.type = "NoSuchSampler"
    with pytest.raises(UnknownType):
        build_disp_sampler(cfg)
    cfg = _settings("configs/DeepPruner/scene_flow_4x.py")
    cfg.model.disp_sampler.propagation_filter_size = 5
    with pytest.raises(NotImplementedError, match="propagation_filter_size"):
        build_disp_sampler(cfg)
    with pytest.raises(NotImplementedError):
        DeepPrunerSampler(max_disp=48, iterations=0)
    with pytest.raises(NotImplementedError):
        DeepPrunerSampler(max_disp=48, patch_match_disparity_sample_number=2)       # no interval between the ends
    with pytest.raises(NotImplementedError):
        DeepPrunerSampler(max_disp=48, patch_match_disparity_sample_number=1000)
    with pytest.raises(NotImplementedError):
        DeepPrunerSampler(max_disp=48, uniform_disparity_sample_number=1)
    assert DeepPrunerSampler(max_disp=48, patch_match_disparity_sample_number=18).patch_match.disparity_sample_number == 18


def test_deeppruner_models_stay_refused():
    from densematchingbenchmark_amd.modeling import build_model
    for rel in ("configs/DeepPruner/scene_flow_4x.py", "configs/DeepPruner/scene_flow_8x.py"):
        with pytest.raises(NotImplementedError):
            build_model(_settings(rel))


def test_no_device_fails_loudly():
    """CPU tensors: the library's binding refuses them; nothing falls back to torch."""
    s = DeepPrunerSampler(max_disp=24)
    left, right, noise, lo, hi = R.golden_inputs("c")
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        s('pre', left, right, noise=noise)
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        s('pre', left, right)
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        s('post', left, right, lo, hi)
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        s.uniform_sampler(lo, hi)


def test_argument_checks_before_the_device():
    s = DeepPrunerSampler(max_disp=24)
    left, right, noise, lo, hi = R.golden_inputs("c")
    for bad in (noise[:, :5], noise.double(), noise[..., :-1], "noise"):
        with pytest.raises(ValueError, match="noise"):
            s('pre', left, right, noise=bad)
    with pytest.raises(NotImplementedError, match="backward"):
        s('pre', left.clone().requires_grad_(), right, noise=noise)
    with pytest.raises(NotImplementedError, match="backward"):
        s('post', left, right, lo.clone().requires_grad_(), hi)
    with pytest.raises(ValueError):
        s('post', left, right)
    lib = _lib.load()
    assert lib.dmb_patch_match_step_f32(None, None, None, None, None, 0.0, 1.0, None, None, 1, 1, 1, 2, 2, 0, 7.0, 1, 0, 0, None) == 100001
    assert lib.dmb_deeppruner_uniform_samples_f32(None, None, None, 1, 2, 2, 9, 1, 24.0, None) == 100001
