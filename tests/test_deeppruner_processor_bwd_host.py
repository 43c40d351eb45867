"""The backward of DeepPruner's cost processor, the parts that need no GPU: the new functions' argument checks (before any launch),
the modules' own refusals (unchanged), the set of exported symbols (unchanged: the feature adds none), and the golden file
tests/golden/deeppruner_processor_bwd.npz against autograd through the restatement of tests/_deeppruner_processor_ref.py on the CPU,
bit for bit."""
import os

import numpy as np
import pytest
import torch

from densematchingbenchmark_amd import _lib
from densematchingbenchmark_amd.modeling.stereo.cost_processors.DeepPruner import ConfidenceRangePredictor, DeepPrunerProcessor
from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
from densematchingbenchmark_amd.modeling.stereo.layers.small_conv5x5 import SmallConv5x5
from tests import _deeppruner_processor_bwd_ref as Q
from tests.test_deeppruner_processor_host import _cfg

GOLDEN = Q.GOLDEN


def _processor(C, P, N):
    return DeepPrunerProcessor(_cfg(C, P, N))


def test_new_functions_refuse_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_launch)
    C, P, N = 4, 5, 3
    proc = _processor(C, P, N)
    crp = proc.confidence_range_predictor
    z = torch.zeros
    # CPU tensors
    for mod in (proc, proc.eval()):
        with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
            train_fn.deeppruner_processor(mod, "pre", z((1, C, 8, 8)), z((1, C, 8, 8)), z((1, P, 8, 8)))
        with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
            train_fn.deeppruner_processor(mod, "post", z((1, C, 8, 8)), z((1, C, 8, 8)), z((1, N, 8, 8)), z((1, P, 8, 8)), z((1, P, 8, 8)))
        with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
            train_fn.confidence_range_predictor(mod.confidence_range_predictor, z((1, 2 * C + 1, P, 8, 8), requires_grad=True), z((1, P, 8, 8)))
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        train_fn.deeppruner_volume(z((1, C, 8, 8)), z((1, C, 8, 8)), z((1, P, 8, 8)))
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        train_fn.small_conv5x5(SmallConv5x5(True, 3, 3), z((1, 3, 8, 8)))
    # a volume whose height or width is no multiple of 8, or with other channels than the predictor's
    for shape in ((1, 2 * C + 1, P, 12, 16), (1, 2 * C + 1, P, 16, 20), (1, 2 * C + 2, P, 16, 16), (2 * C + 1, P, 16, 16)):
        with pytest.raises(ValueError, match="multiples of 8"):
            train_fn.confidence_range_predictor(crp, z(shape), z((1, P) + shape[-2:]))
    wide = train_fn.FAST_FMS_BWD_MAX_W + 8
    gpu = z       # (shapes are checked before devices: CPU tensors reach these refusals)
    for stage, extra in (("pre", ()), ("post", (gpu((1, P, 8, wide)), gpu((1, P, 8, wide))))):
        with pytest.raises(NotImplementedError, match="wider than %d" % train_fn.FAST_FMS_BWD_MAX_W):
            train_fn.deeppruner_processor(proc, stage, gpu((1, C, 8, wide)), gpu((1, C, 8, wide)), gpu((1, P, 8, wide)), *extra)
    with pytest.raises(NotImplementedError, match="wider than %d" % train_fn.FAST_FMS_BWD_MAX_W):
        train_fn.deeppruner_volume(gpu((1, C, 8, wide)), gpu((1, C, 8, wide)), gpu((1, P, 8, wide)))
    for hw in ((12, 16), (16, 20)):
        with pytest.raises(ValueError, match="multiples of 8"):
            train_fn.deeppruner_processor(proc, "pre", gpu((1, C) + hw), gpu((1, C) + hw), gpu((1, P) + hw))
    with pytest.raises(NotImplementedError, match="normalised"):
        train_fn.SoftArgminSampledFn.apply(z((1, 3, 8, 8)), z((1, 3, 8, 8)), False)


def test_module_refusals_are_still_in_place():
    C, P, N = 4, 5, 3
    proc = _processor(C, P, N).eval()
    left, samples = torch.zeros((1, C, 8, 8)), torch.zeros((1, P, 8, 8))
    with pytest.raises(NotImplementedError, match="no backward"):
        proc("pre", left, left, samples)                     # eval(), but grad mode on and the parameters require grad
    with pytest.raises(NotImplementedError, match="no backward"):
        with torch.no_grad():
            proc.train()("pre", left, left, samples)
    crp = ConfidenceRangePredictor(2 * C + 1, 16, P).eval()
    with pytest.raises(NotImplementedError, match="no backward"):
        crp(torch.zeros((1, 2 * C + 1, P, 8, 8)), samples)
    with pytest.raises(NotImplementedError, match="no backward"):
        crp.heads(torch.zeros((1, P, 8, 8), requires_grad=True), torch.zeros((1, P, 8, 8)), samples)
    for conv in (SmallConv5x5(False, 1, 1), SmallConv5x5(True, 3, 3)):
        with pytest.raises(NotImplementedError, match="no backward"):
            conv.eval()(torch.zeros((1, conv.in_planes, 8, 8)))
        with pytest.raises(NotImplementedError, match="no backward"):
            with torch.no_grad():
                conv.train()(torch.zeros((1, conv.in_planes, 8, 8)))
    from densematchingbenchmark_amd.modeling.stereo.cost_processors import PROCESSORS
    assert not any("pruner" in k.lower() for k in PROCESSORS)


def test_the_feature_adds_no_exported_symbol():
    """The 5x5 weight gradient is reached through dmb_conv2d_wgrad_f32, the composed backwards through existing launches."""
    names = _lib.header_symbols()
    assert len(names) == 115 and len(set(names)) == 115   # (113 + the two up-sampling plan queries)
    assert "dmb_conv2d_wgrad_f32" in names and not any("k5" in n and "wgrad" in n for n in names)
    assert _lib.DEFINES["DMB_ABI_VERSION"] == 13


@pytest.mark.parametrize("name,stage,mode", Q.RUNS, ids=["%s-%s-%s" % r for r in Q.RUNS])
def test_golden_file_is_reproduced_by_the_restatement_bit_for_bit(name, stage, mode):
    z = np.load(GOLDEN)
    res = Q.reference(name, stage, mode, torch.float32)
    prefix = "%s/%s/%s/" % (name, stage, mode)
    assert np.array_equal(z[prefix + "loss"], res["loss"].numpy())
    assert sorted(k[len(prefix) + 3:] for k in z.files if k.startswith(prefix + "in/")) == sorted(Q.INPUTS[stage]) == sorted(res["inputs"])
    for k, g in res["inputs"].items():
        assert np.array_equal(z[prefix + "in/" + k], g.numpy()), k
    names, stats, samples = Q.packed(prefix, res["grads"])
    assert list(z[prefix + "p/names"]) == list(names) and len(names) == {"pre": 86, "post": 49}[stage]
    assert np.array_equal(z[prefix + "p/stats"], stats) and np.array_equal(z[prefix + "p/samples"], samples)
    if mode == "train":
        keys = list(z[prefix + "b/names"])
        assert keys and all(k in res["buffers"] for k in keys)
        for i, k in enumerate(keys):
            assert np.array_equal(z[prefix + "b/%d" % i], res["buffers"][k].numpy()), k
    else:
        assert not any(k.startswith(prefix + "b/") for k in z.files)


def test_golden_file_holds_exactly_the_runs():
    z = np.load(GOLDEN)
    assert {tuple(k.split("/")[:3]) for k in z.files} == set(Q.RUNS) and len(Q.RUNS) == 12
    assert os.path.getsize(GOLDEN) < (1 << 20)


def test_the_fp32_restatement_meets_the_whole_network_rule_at_these_seeds():
    for name, stage, mode in Q.GPU_RUNS:
        r32, r64 = Q.reference(name, stage, mode, torch.float32), Q.reference(name, stage, mode, torch.float64)
        t32, t64 = Q.yardstick_tensors(r32, mode), Q.yardstick_tensors(r64, mode)
        n, tight = Q.whole_network_rule(t32, t64, t32, "%s %s %s" % (name, stage, mode))
        zeros = Q.check_zero_grads(r32["grads"], r32["grads"], mode, "%s %s %s" % (name, stage, mode))
        assert n == tight == 1 + {"pre": 86, "post": 49}[stage] - zeros and zeros == {"eval": 0, "train": {"pre": 2, "post": 1}[stage]}[mode]
