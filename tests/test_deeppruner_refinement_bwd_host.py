"""The backward of DeepPruner's refinement, the parts that need no GPU: the new functions' refusals (before any launch), the
modules' own refusals and the registries (unchanged), the set of exported symbols (unchanged: the feature adds none), and the
golden file tests/golden/deeppruner_refinement_bwd.npz against autograd through the restatement of
tests/_deeppruner_features_ref.py on the CPU, bit for bit."""
import os

import numpy as np
import pytest
import torch

from densematchingbenchmark_amd import _lib
from densematchingbenchmark_amd.modeling.stereo.disp_refinement import REFINEMENTS, DeepPrunerRefinement, RefinementHeand
from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
from tests import _deeppruner_features_ref as R
from tests import _deeppruner_refinement_bwd_ref as Q
from tests._hw_bwd_ref import whole_network_rule

N_PARAMS = {"r4x": 19, "r8x": 38, "rodd": 19}      # per stage: six convolutions, six BatchNorm pairs, the classifier


def test_new_functions_refuse_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_launch)
    z = torch.zeros
    ref = DeepPrunerRefinement([7], True, 1)
    for training in (True, False):
        mod = ref.train(training)
        assert mod.training == training and mod.refine_blocks[0].conv[0].training == training
        with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
            train_fn.deeppruner_refinement(mod, [z((1, 1, 5, 13))], [z((1, 6, 5, 13), requires_grad=True)])
        with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
            train_fn.refinement_head(mod.refine_blocks[0], z((1, 1, 5, 13)), z((1, 16, 5, 13)))
    block = ref.refine_blocks[0]
    for init, guide in ((z((1, 1, 5, 13)), z((1, 15, 5, 13))), (z((1, 1, 5, 12)), z((1, 16, 5, 13))), (z((1, 2, 5, 13)), z((1, 16, 5, 13))),
                        (z((2, 1, 5, 13)), z((1, 16, 5, 13))), (z((1, 5, 13)), z((16, 5, 13)))):
        with pytest.raises(ValueError, match="refinement_head"):
            train_fn.refinement_head(block, init, guide)


def test_double_backward_is_refused():
    """``_refuse_double_backward`` is the first statement of RefineHeadFn.backward and of RefineStageFn.backward"""
    class Ctx:
        what = "deeppruner_refinement"
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="double backward"):
            train_fn.RefineHeadFn.backward(Ctx(), torch.zeros((1, 1, 2, 2)))
        with pytest.raises(NotImplementedError, match="deeppruner_refinement: double backward"):
            train_fn.RefineStageFn.backward(Ctx(), torch.zeros((1, 1, 2, 2)))


def test_module_refusals_and_registries_are_unchanged():
    ref = DeepPrunerRefinement([7], True, 1).eval()
    disp, fms = torch.zeros((1, 1, 5, 13)), torch.zeros((1, 6, 5, 13))
    with pytest.raises(NotImplementedError, match="the fused refinement head has none"):
        ref([disp], [fms])                           # eval(), but grad mode on and the parameters require grad
    with pytest.raises(NotImplementedError, match="the fused refinement head has none"):
        with torch.no_grad():
            ref.train()([disp], [fms])
    head = RefinementHeand(7).eval()
    with pytest.raises(NotImplementedError, match="the fused refinement head has none"):
        head(disp, torch.zeros((1, 7, 5, 13)))
    with pytest.raises(NotImplementedError, match="the fused refinement head has none"):
        head.classify(torch.zeros((1, 16, 5, 13), requires_grad=True), disp)
    assert REFINEMENTS["DeepPruner"] is DeepPrunerRefinement and sorted(REFINEMENTS) == ["DeepPruner", "StereoNet"]
    from densematchingbenchmark_amd.modeling.stereo.cost_processors import PROCESSORS
    assert sorted(PROCESSORS) == ["Concatenation", "Correlation", "Difference"]


def test_the_feature_adds_no_exported_symbol():
    """The one-output-channel weight gradient is reached through dmb_conv2d_wgrad_f32, the rest through existing launches."""
    names = _lib.header_symbols()
    assert len(names) == 115 and len(set(names)) == 115
    assert "dmb_conv2d_wgrad_f32" in names and not any("c1" in n and "conv2d" in n for n in names)
    assert _lib.DEFINES["DMB_ABI_VERSION"] == 13


@pytest.mark.parametrize("name,mode", Q.RUNS, ids=["%s-%s" % r for r in Q.RUNS])
def test_golden_file_is_reproduced_by_the_restatement_bit_for_bit(name, mode):
    z = np.load(Q.GOLDEN)
    res = Q.reference(name, mode, torch.float32)
    prefix = "%s/%s/" % (name, mode)
    assert np.array_equal(z[prefix + "loss"], res["loss"].numpy())
    assert list(res["inputs"]) == list(Q.inputs_of(name))
    assert np.array_equal(z[prefix + "in/disp"], res["inputs"]["disp"].numpy())
    fms = {k: g for k, g in res["inputs"].items() if k != "disp"}
    names, stats, samples = Q.packed(prefix, fms, Q.IN_SAMPLES)
    assert list(z[prefix + "in/names"]) == list(names) == list(Q.inputs_of(name)[1:])
    assert np.array_equal(z[prefix + "in/stats"], stats) and np.array_equal(z[prefix + "in/samples"], samples)
    names, stats, samples = Q.packed(prefix, res["grads"])
    assert list(z[prefix + "p/names"]) == list(names) and len(names) == N_PARAMS[name]
    assert np.array_equal(z[prefix + "p/stats"], stats) and np.array_equal(z[prefix + "p/samples"], samples)
    if mode == "train":
        keys = list(z[prefix + "b/names"])
        assert keys == list(res["buffers"]) and len(keys) == 18 * R.REFINE_CASES[name][0][1]
        for i, k in enumerate(keys):
            assert np.array_equal(z[prefix + "b/%d" % i], res["buffers"][k].numpy()), k
    else:
        assert not any(k.startswith(prefix + "b/") for k in z.files)


def test_golden_file_holds_exactly_the_runs():
    z = np.load(Q.GOLDEN)
    assert {tuple(k.split("/")[:2]) for k in z.files} == set(Q.RUNS) and len(Q.RUNS) == 6
    assert os.path.getsize(Q.GOLDEN) < 400 * 1024


def test_the_fp32_restatement_meets_the_whole_network_rule_at_these_seeds():
    for name, mode in Q.GPU_RUNS:
        r32, r64 = Q.reference(name, mode, torch.float32), Q.reference(name, mode, torch.float64)
        n, tight = whole_network_rule(Q.tensors(r32), Q.tensors(r64), Q.tensors(r32), "%s %s" % (name, mode))
        assert n == tight == len(Q.inputs_of(name)) + N_PARAMS[name]
        # every input gets a gradient, and the incoming disparity's is not just the projection of its own place in the list
        own = Q.projections(name, r64["outs"])[-1].double()
        assert (r64["inputs"]["disp"] - own).abs().max().item() > 1e-3
