"""The backward of DeepPruner's sampler on the CPU: imports and refusals (all before the library is loaded), the header against the
ctypes table, the entry points' argument checks without a device, and the yardstick of the GPU tests -- the restatement's autograd
(tests/_deeppruner_ref.py) -- pinned to the real reference's recorded gradients (tests/golden/deeppruner_sampler_grads.npz,
scripts/gen_golden_deeppruner_sampler_grads.py)."""
import os

import numpy as np
import pytest
import torch

from densematchingbenchmark_amd import _lib, ops, ops_deeppruner
from densematchingbenchmark_amd.modeling.stereo.disp_samplers import DeepPrunerSampler
from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
from tests import _deeppruner_ref as R
from tests import _deeppruner_sampler_bwd_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "deeppruner_sampler_grads.npz")
EINVAL, EUNSUPPORTED = 100001, 100002


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", refuse)


def test_public_names():
    assert issubclass(train_fn.PatchMatchFn, torch.autograd.Function) and issubclass(train_fn.UniformSamplesFn, torch.autograd.Function)
    assert callable(train_fn.deeppruner_sampler)
    assert ops.patch_match_step_bwd is ops_deeppruner.patch_match_step_bwd
    assert ops.deeppruner_uniform_samples_bwd is ops_deeppruner.deeppruner_uniform_samples_bwd
    with pytest.raises(AttributeError):
        ops.no_such_wrapper
    assert {"patch_match_step_bwd", "deeppruner_uniform_samples_bwd", "patch_match_step"} <= set(dir(ops))
    assert train_fn.PATCH_MATCH_BWD_MAX_W == ops_deeppruner.PATCH_MATCH_BWD_MAX_W == _lib.DEFINES["DMB_PATCH_MATCH_BWD_MAX_W"] == 1024


def test_refusals_fire_before_the_library(no_library):
    s = DeepPrunerSampler(max_disp=24)
    left, right, noise, lo, hi = R.golden_inputs("c")
    with pytest.raises(NotImplementedError, match="range"):
        train_fn.deeppruner_sampler(s, 'pre', left, right, lo.clone().requires_grad_(), hi, noise=noise)
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        train_fn.deeppruner_sampler(s, 'pre', left.clone().requires_grad_(), right, noise=noise)
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        train_fn.deeppruner_sampler(s, 'pre', left, right)
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        train_fn.deeppruner_sampler(s, 'post', left, right, lo.clone().requires_grad_(), hi)
    with pytest.raises(ValueError):
        train_fn.deeppruner_sampler(s, 'post', left, right)
    with pytest.raises(ValueError, match="noise"):
        train_fn.deeppruner_sampler(s, 'pre', left, right, noise=noise[:, :5])
    wide = torch.zeros((1, 2, 2, 1025))
    with pytest.raises(NotImplementedError, match="1024"):
        train_fn.deeppruner_sampler(s, 'pre', wide, wide)
    with pytest.raises(NotImplementedError, match="1024"):
        ops.patch_match_step_bwd(wide, wide, torch.zeros((1, 12, 2, 1025)), grad_noise=torch.zeros((1, 12, 2, 1025)))
    with pytest.raises(NotImplementedError, match="H, W >= 2"):
        train_fn.deeppruner_sampler(s, 'pre', left[..., :1], right[..., :1])
    # the wrappers check their operands like the forward's and refuse CPU tensors at the binding
    with pytest.raises(_lib.DmbLibraryError, match="noise must be"):
        ops.patch_match_step_bwd(left, right, noise[..., :-1], grad_noise=noise)
    with pytest.raises(_lib.DmbLibraryError, match="neither"):
        ops.patch_match_step_bwd(left, right, noise)
    with pytest.raises(_lib.DmbLibraryError, match="grad_samples must be"):
        ops.patch_match_step_bwd(left, right, noise, grad_samples=noise[:, :3])
    with pytest.raises(_lib.DmbLibraryError, match="both range maps"):
        ops.patch_match_step_bwd(left, right, noise, lo, None, grad_noise=noise)
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        ops.patch_match_step_bwd(left, right, noise, grad_noise=noise)
    with pytest.raises(_lib.DmbLibraryError, match="grad_out must be"):
        ops.deeppruner_uniform_samples_bwd(lo, hi, noise[..., :-1])
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        ops.deeppruner_uniform_samples_bwd(lo, hi, noise, 24.0)


def test_double_backward_is_refused_by_both_functions(no_library, monkeypatch):
    """``create_graph=True`` with an upstream gradient that requires NO gradient itself (a gradient penalty): the backward of
    either Function refuses before it launches anything -- it would return a first gradient without a graph and the second-order
    term would be dropped silently.  The forward launches are stood in for by the restatement on the CPU; the backward wrappers
    must never be reached."""
    def never(*a, **k):
        raise AssertionError("a backward launch was reached")
    monkeypatch.setattr(train_fn.ops_deeppruner, "patch_match_step_bwd", never)
    monkeypatch.setattr(train_fn.ops_deeppruner, "deeppruner_uniform_samples_bwd", never)
    monkeypatch.setattr(train_fn.ops, "deeppruner_uniform_samples",
                        lambda lo, hi, n, max_disp: R.sampler('post', None, None, lo.detach(), hi.detach(), max_disp=max_disp,
                                                              uniform_sample_number=n))

    def fake_step(left, right, noise, lo, hi, vertical, temperature, bounds, want_noise, out):
        if out is not None:
            out.zero_()
        return out, (noise * 0.5 if want_noise else None)
    monkeypatch.setattr(train_fn.ops, "patch_match_step", fake_step)
    lo, hi, g = K.post_inputs("n3")
    a, b = lo.clone().requires_grad_(), hi.clone().requires_grad_()
    out = train_fn.UniformSamplesFn.apply(a, b, 3, 24.0)
    assert out.requires_grad and not g.requires_grad
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(out, (a, b), g, create_graph=True)
    left, right, noise, gp = K.chain_inputs("h6w10", 1)
    left.requires_grad_()
    out = train_fn.PatchMatchFn.apply(left, right, noise, None, None, (0.0, 8.0), 3, 7)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(out, left, gp, create_graph=True)
    with pytest.raises(AssertionError, match="backward launch"):      # without create_graph the backward goes on to its launches
        torch.autograd.grad(out, left, gp)


def test_the_modules_own_forward_still_refuses_gradients(no_library):
    s = DeepPrunerSampler(max_disp=24)
    left, right, noise, lo, hi = R.golden_inputs("c")
    with pytest.raises(NotImplementedError, match="backward"):
        s('pre', left.clone().requires_grad_(), right, noise=noise)
    with pytest.raises(NotImplementedError, match="backward"):
        s.patch_match(left, right.clone().requires_grad_(), noise=noise)
    with pytest.raises(NotImplementedError, match="backward"):
        s('post', left, right, lo.clone().requires_grad_(), hi)
    with pytest.raises(NotImplementedError, match="backward"):
        s.uniform_sampler(lo, hi.clone().requires_grad_())


def test_header_and_ctypes_table():
    names = ("dmb_patch_match_step_bwd_f32", "dmb_deeppruner_uniform_samples_bwd_f32")
    assert _lib.ABI_VERSION == 13
    assert set(names) <= set(_lib.header_symbols()) and set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    for n in names:
        assert n in _lib._LAUNCH
    params = [p for _, p in _lib.PROTOTYPES[names[0]][1]]
    assert params[:3] == ["L", "R", "noise_in"] and params[-1] == "stream" and "workspace" in params and len(params) == 25
    assert [p for _, p in _lib.PROTOTYPES[names[1]][1]] == ["min_disp", "max_disp", "d_out", "d_min", "d_max", "B", "H", "W", "N",
                                                          "range_head", "max_disp_limit", "stream"]
    # the forwards' signatures are untouched
    assert len(_lib.PROTOTYPES["dmb_patch_match_step_f32"][1]) == 20 and len(_lib.PROTOTYPES["dmb_deeppruner_uniform_samples_f32"][1]) == 10


def test_entry_points_check_their_arguments_without_a_device():
    import ctypes
    lib = _lib.load()
    p = ctypes.c_void_p(0x1000)          # never dereferenced: every call below is refused before a launch

    def step(L=p, g_samples=p, g_noise=None, dL=p, ws=p, min_disp=None, max_disp=None, B=1, C=4, P=3, H=4, W=8, ctot=3, coff=0):
        return lib.dmb_patch_match_step_bwd_f32(L, p, p, min_disp, max_disp, 0.0, 8.0, g_samples, g_noise, None, None, dL, p, p, ws,
                                                B, C, P, H, W, 0, 7.0, ctot, coff, None)
    assert step(L=None) == EINVAL and step(g_samples=None) == EINVAL and step(dL=None) == EINVAL and step(ws=None) == EINVAL
    assert step(min_disp=p) == EINVAL and step(B=0) == EINVAL and step(P=0) == EINVAL
    assert step(ctot=3, coff=1) == EINVAL and step(coff=-1) == EINVAL
    assert step(W=1) == EUNSUPPORTED and step(H=1) == EUNSUPPORTED
    assert step(P=_lib.DEFINES["DMB_PATCH_MATCH_MAX_SAMPLES"] + 1, ctot=200) == EUNSUPPORTED
    assert step(W=1025) == EUNSUPPORTED and step(B=70000) == EUNSUPPORTED and step(C=1 << 20, H=64, W=64) == EUNSUPPORTED

    def uni(d_out=p, d_min=p, lo=p, N=9, head=1, B=1):
        return lib.dmb_deeppruner_uniform_samples_bwd_f32(lo, p, d_out, d_min, p, B, 4, 8, N, head, 24.0, None)
    assert uni(d_out=None) == EINVAL and uni(d_min=None) == EINVAL and uni(lo=None) == EINVAL and uni(B=0) == EINVAL
    assert uni(N=1) == EUNSUPPORTED and uni(N=_lib.DEFINES["DMB_MAX_DISP_SAMPLES"] + 1) == EUNSUPPORTED and uni(B=70000) == EUNSUPPORTED


def test_restatement_autograd_meets_the_reference_recording():
    """FP32 autograd through the restatement against the real reference's recorded gradients, by the GPU tests' own rule with the
    recording in the place of the device result: the yardstick is the reference."""
    z = np.load(GOLDEN)
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    fails = []
    try:
        for name in K.CHAIN_CASES:
            seed = K.chain_seed(name)
            assert int(z[name + "/seed"]) == seed, name
            assert torch.equal(K.chain_inputs(name, seed)[3], torch.from_numpy(z[name + "/g"]))
            r64, r32 = K.chain_grads(name, seed, torch.float64), K.chain_grads(name, seed, torch.float32)
            assert torch.equal(r32[0], torch.from_numpy(z[name + "/pre"])), name     # the forward: bit for bit
            K.bound_check(name + " d_left", torch.from_numpy(z[name + "/d_left"]), r64[1], r32[1], fails)
            K.bound_check(name + " d_right", torch.from_numpy(z[name + "/d_right"]), r64[2], r32[2], fails)
            assert (r32[0].double() - r64[0]).abs().max().item() <= 4e-6 * r64[0].abs().max().item(), name
        for name, (shape, N, max_disp, _) in K.POST_CASES.items():
            lo, hi, g = K.post_inputs(name)
            assert torch.equal(g, torch.from_numpy(z[name + "/g"]))
            r64, r32 = K.post_grads(lo, hi, g, N, max_disp, torch.float64), K.post_grads(lo, hi, g, N, max_disp, torch.float32)
            assert torch.equal(r32[0], torch.from_numpy(z[name + "/post"])), name
            K.bound_check(name + " d_lo", torch.from_numpy(z[name + "/d_lo"]), r64[1], r32[1], fails)
            K.bound_check(name + " d_hi", torch.from_numpy(z[name + "/d_hi"]), r64[2], r32[2], fails)
    finally:
        torch.set_num_threads(threads)
    assert not fails, "\n".join(fails)


def test_case_constructions_keep_their_margins():
    """The cell rule and the decision margins hold for what the GPU tests run on (and the constructions converge)."""
    for name in K.CHAIN_CASES:
        assert K.chain_margin(name, K.chain_seed(name)) >= K.CHAIN_MARGIN
    left, right, noise, lo, hi, _, _ = K.step_inputs((2, 8, 9, 23), 3, 11, True, True, 5)
    assert K.cell_margin(K.candidate_ix(noise.double(), lo.double(), hi.double(), True)).min().item() >= 1e-3
    ix = K.candidate_ix(noise.double(), lo.double(), hi.double(), True)
    assert (ix < -1).any() and (ix > 23).any()              # x - s leaves the image on both sides
    for name, (shape, N, max_disp, _) in K.POST_CASES.items():
        lo, hi, _ = K.post_inputs(name)
        assert K.post_decisions(lo.double(), hi.double(), N, max_disp).abs().min().item() >= K.POST_MARGIN
