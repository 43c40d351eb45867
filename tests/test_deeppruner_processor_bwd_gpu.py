"""The backward of DeepPruner's cost processor on the MI355X (layers/train_fn.py: ``small_conv5x5``, ``SoftArgminSampledFn``,
``deeppruner_volume``, ``confidence_range_predictor`` and ``deeppruner_processor``).

UNITS -- one SmallConv5x5 through ``train_fn.small_conv5x5`` (the module's own ``forward`` stays inference only) against the unit's
own torch children on the CPU in FP64 and FP32, with the machinery of tests/test_unit_grads_gpu.py: the upstream gradient is zero
wherever the FP64 pre-activation of the ReLU lies within MARGIN x max of zero, so the ReLU cannot flip and EVERY tensor (output, dx,
dw, dbias, dgamma, dbeta) is held to |hip - fp64| <= 4 |fp32 - fp64| + 2e-6 x range; running buffers within 1e-5 relative; a second
pass bit-identical.  The share of upstream elements the margin zeroes is asserted below 1 % per case.  Per (unit, shape): BatchNorm
none / batch statistics / running statistics x the gradient carry on / off (1 -> 1: a bias and no BatchNorm, as the model has it).

SOFT ARG-MIN and VOLUME -- the two composed backwards alone, against CPU autograd through the restatement's ``soft_argmin`` (tight
rule) and ``raw_volume`` (the rules of test_fast_volume_builders_backward_through_the_samples, on its inputs).

NETWORKS -- ``deeppruner_processor`` in both stages (stage "pre" is the volume and ``confidence_range_predictor``) against autograd
through tests/_deeppruner_processor_ref.py (tests/_deeppruner_processor_bwd_ref.py: runs, loss, rules), in eval() with trainable
weights and, on case a, in train().  A ReLU inside the network may flip, so the rule is the whole-network rule of
tests/test_backward_gpu.py -- every gradient within 3e-2 of its range, at least 60 % of the tensors within 4 |fp32 - fp64| + 2e-5 x
range -- for the raw volume's gradient and every parameter's, which is what the FP64 yardstick covers (it starts after the volume);
the recorded gradients of the real reference (tests/golden/deeppruner_processor_bwd.npz) are matched under the same rule.  The
gradients of left, right, the samples and the two feature maps are held to the FP32 restatement, which the recording equals bit for
bit."""
import numpy as np
import pytest
import torch

from tests import _deeppruner_processor_bwd_ref as Q
from tests import _deeppruner_processor_ref as R
from tests.test_backward_gpu import _close
from tests.test_deeppruner_processor_gpu import _cfg, _check, _factor
from tests.test_unit_grads_gpu import MARGIN, _buffers, _compare, _init, _leaves, _params, _pass, _RefUnit, _Toggles

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------- units
UNITS = {"c1": 1, "c2": 2, "c9": 9, "c14": 14}                 # channels in = channels out
SHAPES = {"a": (2, 8, 16), "odd": (2, 7, 13), "b": (2, 16, 40)}     # (B, H, W)
UNIT_CASES = [(u, s) for u in UNITS for s in SHAPES]


def _make_unit(name, bn, dev, g):
    from densematchingbenchmark_amd.modeling.stereo.layers.small_conv5x5 import SmallConv5x5
    m = SmallConv5x5(bn != "none", UNITS[name], UNITS[name], bias=True)
    _init([m], g)
    m = m.to(dev).train(bn == "train")
    for p in m.parameters():
        p.requires_grad_(True)
    return [m]


def _call(m, t):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    return [m[0](t["x"], relu=True) if isinstance(m[0], _RefUnit) else train_fn.small_conv5x5(m[0], t["x"])]


def _check_unit(mods, t64, carry, dev, g):
    """tests/test_deeppruner_aggregator_bwd_gpu.py: _check_units, for one SmallConv5x5"""
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    fails = []
    ref64, ref32 = [_RefUnit(m, torch.float64) for m in mods], [_RefUnit(m, torch.float32) for m in mods]
    saved = [{k: v.detach().clone() for k, v in _buffers(m).items()} for m in mods]
    t_64 = _leaves(t64, torch.float64, "cpu")
    outs64 = _call(ref64, t_64)
    pre = ref64[0].pre.detach()
    gi = torch.randn(outs64[0].shape, generator=g, dtype=torch.float64)
    mask = pre.abs() < MARGIN * pre.abs().max()
    gi[mask] = 0.0
    assert int(mask.sum()) < 0.01 * gi.numel(), "the margin zeroes %d of %d upstream elements" % (int(mask.sum()), gi.numel())
    gs = [gi]
    torch.autograd.backward(outs64, gs)
    grads64 = {("in", k): v.grad for k, v in t_64.items()}
    for n, p in _params(ref64[0]).items():
        grads64[(0, n)] = p.grad
    outs32, grads32 = _pass(ref32, _call, _leaves(t64, torch.float32, "cpu"), gs)
    runs = []
    for rep in range(2):
        if rep:
            with torch.no_grad():
                for m, s in zip(mods, saved):
                    for k, v in _buffers(m).items():
                        if not torch.equal(v, s[k].to(v.device)):
                            v.copy_(s[k])
        with _Toggles(dict(split_k=True, carry=carry, pack_group=True, epilogue=False)):
            outs, grads = _pass(mods, _call, _leaves(t64, torch.float32, dev), gs, train_fn.carry_scope)
        torch.cuda.synchronize()
        bufs = [{k: v.detach().cpu().clone() for k, v in _buffers(m).items()} for m in mods]
        runs.append(([o.detach().cpu() for o in outs], {k: (v.detach().cpu() if v is not None else None) for k, v in grads.items()}, bufs))
        if rep == 0 and type(outs[0].grad_fn).__name__ != "SmallConv5x5FnBackward":
            fails.append("output made by %s" % type(outs[0].grad_fn).__name__)
    (outs, grads, bufs), (outs2, grads2, _) = runs
    gmax = max([v.detach().abs().max().item() for v in grads64.values() if v is not None and v.numel()] + [0.0])
    _compare("output", outs[0], outs64[0], outs32[0], 0.0, fails)
    assert set(grads) == set(grads64)
    for k in grads64:
        _compare("d%s" % (k,), grads.get(k), grads64[k], grads32[k], 1e-6 * gmax, fails)
    for k, v64 in _buffers(ref64[0]).items():
        b = bufs[0][k]
        if v64.dtype == torch.int64:
            if not torch.equal(b, v64):
                fails.append("%s: %s != %s" % (k, b.tolist(), v64.tolist()))
        elif not (b.double() - v64).abs().max().item() <= 1e-5 * max(v64.abs().max().item(), 1e-2):
            fails.append("%s: error %.3e" % (k, (b.double() - v64).abs().max().item()))
    if not torch.equal(outs[0], outs2[0]):
        fails.append("second pass: output differs")
    for k, v in grads.items():
        if (v is None) != (grads2[k] is None) or (v is not None and not torch.equal(v, grads2[k])):
            fails.append("second pass: d%s not bit-identical" % (k,))
    return fails


@pytest.mark.parametrize("name,shape", UNIT_CASES, ids=["%s-%s" % c for c in UNIT_CASES])
def test_small_conv5x5_forward_and_backward_against_fp64(dev, name, shape):
    B, H, W = SHAPES[shape]
    failures = []
    options = ("none",) if name == "c1" else ("none", "train", "eval")
    for n, (bn, carry) in enumerate((b, c) for b in options for c in (True, False)):
        g = torch.Generator().manual_seed(96000 + 100 * list(UNITS).index(name) + 10 * list(SHAPES).index(shape) + n)
        mods = _make_unit(name, bn, dev, g)
        t64 = {"x": torch.randn((B, UNITS[name], H, W), generator=g, dtype=torch.float64)}
        failures += ["%s carry %s: %s" % (bn, carry, f) for f in _check_unit(mods, t64, carry, dev, g)]
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------- soft arg-min
@pytest.mark.parametrize("D", [2, 9, 14])
@pytest.mark.parametrize("hw", [(8, 16), (7, 13)], ids=["8x16", "7x13"])
def test_soft_argmin_sampled_backward_against_fp64(dev, D, hw):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    H, W = hw
    g = torch.Generator().manual_seed(97000 + 10 * D + H)
    cost = torch.randn((2, D, H, W), generator=g)
    sample = torch.sort(torch.rand((2, D, H, W), generator=g) * (W / 2.0), dim=1)[0]
    up = torch.randn((2, 1, H, W), generator=g)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        c, s = cost.to(dtype, copy=True).requires_grad_(), sample.to(dtype, copy=True).requires_grad_()
        out = R.soft_argmin(c, s)
        out.backward(up.to(dtype))
        ref[dtype] = (out.detach(), c.grad, s.grad)
    runs = []
    for _ in range(2):
        c, s = cost.to(dev).requires_grad_(), sample.to(dev).requires_grad_()
        out = train_fn.SoftArgminSampledFn.apply(c, s)
        out.backward(up.to(dev))
        runs.append((out.detach(), c.grad, s.grad))
    for what, got, r64, r32 in zip(("disparity", "d cost", "d sample"), runs[0], ref[torch.float64], ref[torch.float32]):
        _close(got.cpu(), r64, r32, "D %d %dx%d %s" % (D, H, W, what))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "a second pass must be bit-identical"
    with pytest.raises(NotImplementedError, match="double backward"):
        c = cost.to(dev).requires_grad_()
        torch.autograd.grad(train_fn.SoftArgminSampledFn.apply(c, sample.to(dev)).sum(), c, create_graph=True)


# ------------------------------------------------------------------------------------------------------------- the volume
@pytest.mark.parametrize("P", [0, 3])
def test_volume_function_against_autograd_through_the_restatement(dev, P):
    """Inputs as in test_fast_volume_builders_backward_through_the_samples (tests/golden/fast_volumes_grad.npz: shapes, sample
    count, seeds).  Every gradient within 2e-5 x scale of CPU autograd through ``raw_volume`` in FP32, and no further from the
    FP64 one than max(4 x the FP32 one's distance, 1e-6 x scale); the range features' gradients equal the ascending-plane loop."""
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    from tests._util import golden
    from tests.test_kernels_gpu import _rand
    cases = golden("fast_volumes_grad.npz")["cases"]
    for i, row in enumerate(cases):
        sh, D, seed = tuple(int(v) for v in row[:4]), int(row[4]), int(row[5])
        B, C, H, W = sh
        a, b = _rand(sh, seed), _rand(sh, seed + 1000)
        gen = torch.Generator().manual_seed(seed + 2000)
        ds = torch.rand((B, D, H, W), generator=gen) * W * 0.6 - 2.0
        feats = [_rand((B, P, H, W), seed + 4000 + j) for j in range(2)] if P else []
        up = _rand((B, 2 * C + 1 + 2 * P, D, H, W), seed + 3000)
        names = ["dL", "dR", "dS"] + (["dmin", "dmax"] if P else [])
        ref = {}
        for dtype in (torch.float64, torch.float32):
            leaves = [t.to(dtype, copy=True).requires_grad_() for t in [a, b, ds] + feats]
            R.raw_volume(*leaves).backward(up.to(dtype))
            ref[dtype] = [t.grad for t in leaves]
        leaves = [t.to(dev).requires_grad_() for t in [a, b, ds] + feats]
        vol = train_fn.deeppruner_volume(*leaves)
        with torch.no_grad():
            assert torch.equal(vol.cpu(), R.raw_volume(*([a, b, ds] + feats))), "the forward is the restatement's, bit for bit"
        vol.backward(up.to(dev))
        for key, leaf, r64, r32 in zip(names, leaves, ref[torch.float64], ref[torch.float32]):
            got = leaf.grad.cpu()
            scale = max(1.0, r32.abs().max().item())
            assert got.shape == r32.shape
            assert (got - r32).abs().max().item() <= 2e-5 * scale, (key, i)
            e_got, e_ref = (got.double() - r64).abs().max().item(), (r32.double() - r64).abs().max().item()
            print("case %d P %d %s: e_hip %.3g e_fp32 %.3g scale %.3g" % (i, P, key, e_got, e_ref, scale))
            assert e_got <= max(4 * e_ref, 1e-6 * scale), (key, i, e_got, e_ref)
        for j in range(2 if P else 0):
            c0 = 2 * C + 1 + j * P
            acc = up[:, c0:c0 + P, 0].clone()
            for d in range(1, D):
                acc += up[:, c0:c0 + P, d]
            assert torch.equal(leaves[3 + j].grad.cpu(), acc), "d %s_feature: the planes are added in ascending order" % ("min", "max")[j]
    # only the samples want a gradient
    S = ds.to(dev).requires_grad_()
    train_fn.deeppruner_volume(a.to(dev), b.to(dev), S, *[f.to(dev) for f in feats]).backward(up.to(dev))
    assert torch.equal(S.grad, leaves[2].grad)


# ------------------------------------------------------------------------------------------------------------- networks
def _hip_processor(name, mode, dev):
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.DeepPruner import DeepPrunerProcessor
    (B, C, P, N, H, W), _ = R.CASES[name]
    return Q.fill(DeepPrunerProcessor(_cfg(C, P, N))).to(dev).train(mode == "train")


def _hip_run(monkeypatch, name, stage, mode, dev, mod=None):
    """Q.run through train_fn.deeppruner_processor, with the raw volume's gradient kept"""
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    seen, volume = [], train_fn.deeppruner_volume

    def spy(*args):
        v = volume(*args)
        v.retain_grad()
        seen.append(v)
        return v
    monkeypatch.setattr(train_fn, "deeppruner_volume", spy)
    mod = mod if mod is not None else _hip_processor(name, mode, dev)
    res = Q.run(mod, name, stage, forward=train_fn.deeppruner_processor, device=dev)
    torch.cuda.synchronize()
    monkeypatch.setattr(train_fn, "deeppruner_volume", volume)
    assert len(seen) == 1
    res["draw"], res["raw"] = seen[0].grad, seen[0].detach()
    return mod, res


@pytest.mark.parametrize("name,stage,mode", Q.GPU_RUNS, ids=["%s-%s-%s" % r for r in Q.GPU_RUNS])
def test_processor_against_autograd_through_the_restatement(dev, monkeypatch, name, stage, mode):
    what = "%s %s %s" % (name, stage, mode)
    mod = _hip_processor(name, mode, dev)
    before = {k: v.detach().clone() for k, v in mod.named_buffers()}
    mod, res = _hip_run(monkeypatch, name, stage, mode, dev, mod)
    r64, r32 = Q.reference(name, stage, mode, torch.float64), Q.reference(name, stage, mode, torch.float32)
    with torch.no_grad():
        assert torch.equal(res["raw"].cpu(), R.raw_volume(*[Q.case_tensors(name, stage)[k] for k in Q.INPUTS[stage]]))
    keys = R.OUTPUTS[:4] if stage == "pre" else R.OUTPUTS[4:]
    assert len(res["outs"]) == len(keys)
    for key, o, o32, o64 in zip(keys, res["outs"], r32["outs"], r64["outs"]):      # the forward contract of the eval path
        _check(o, o32, o64, "%s %s" % (what, key), _factor(key))
    # the loss, a sum: 4x the FP32 restatement's own error plus 2e-6 of the sum of its terms' magnitudes
    mass = sum((o * p.double()).abs().sum().item() for o, p in zip(r64["outs"], Q.projections(name, stage, r64["outs"])))
    assert abs(res["loss"].item() - r64["loss"].item()) <= 4 * abs(r32["loss"].item() - r64["loss"].item()) + 2e-6 * mass
    # what the FP64 yardstick covers: d raw_cost and the parameters
    n_params = {"pre": 86, "post": 49}[stage]
    assert sorted(res["grads"]) == sorted(r64["grads"]) and len(res["grads"]) == n_params
    zeros = Q.check_zero_grads(res["grads"], r32["grads"], mode, what)
    n, tight = Q.whole_network_rule(Q.yardstick_tensors(res, mode), Q.yardstick_tensors(r64, mode), Q.yardstick_tensors(r32, mode), what)
    print("%s: %d of %d gradients within the tight bound" % (what, tight, n))
    assert n == 1 + n_params - zeros
    # the inputs: the FP32 restatement (= the recording, bit for bit: tests/test_deeppruner_processor_bwd_host.py)
    Q.coarse_rule(res["inputs"], r32["inputs"], what + " inputs")
    z = np.load(Q.GOLDEN)
    prefix = "%s/%s/%s/" % (name, stage, mode)
    Q.coarse_rule(res["inputs"], {k: torch.from_numpy(z[prefix + "in/" + k]) for k in Q.INPUTS[stage]}, what + " inputs against the recording")
    # the recorded parameter gradients of the real reference under the whole-network rule (the recording stands in for FP32)
    names = [str(k) for k in z[prefix + "p/names"]]
    assert names == list(r64["grads"])
    gold = {k: torch.from_numpy(z[prefix + "p/samples"][i][:min(Q.SAMPLES, r64["grads"][k].numel())]) for i, k in enumerate(names)}
    live = {k: v for k, v in res["grads"].items() if not Q.zero_by_construction(k, mode)}
    got, ref = Q.sampled(prefix, live), Q.sampled(prefix, {k: r64["grads"][k] for k in live})
    Q.whole_network_rule(got, ref, {k: gold[k] for k in live}, what + " against the recording")
    for k, v in mod.named_buffers():
        if mode == "eval" or not any(k.startswith(u + ".") for u in {p.rsplit(".", 2)[0] for p in res["grads"]}):
            assert torch.equal(v, before[k]), k
        else:
            want = r64["buffers"][k]
            assert (v.cpu().double() - want.double()).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item()), k


def test_a_second_pass_is_bit_identical_but_for_the_target_feature(dev, monkeypatch):
    """``fast_fms_bwd`` sums the target feature's gradient with LDS atomics (the exception the memory-contract tests make too)"""
    for name, stage, mode in (("b", "pre", "eval"), ("c", "post", "eval"), ("a", "post", "train")):
        runs = [_hip_run(monkeypatch, name, stage, mode, dev)[1] for _ in range(2)]     # (train(): the buffers start from the same values)
        a, b = runs
        assert all(torch.equal(x, y) for x, y in zip(a["outs"], b["outs"])) and torch.equal(a["draw"], b["draw"]), (name, stage, mode)
        for k in Q.INPUTS[stage]:
            if k == "right":
                scale = a["inputs"][k].abs().max().item()
                assert (a["inputs"][k] - b["inputs"][k]).abs().max().item() <= 1e-5 * scale, (name, stage, mode, k)
            else:
                assert torch.equal(a["inputs"][k], b["inputs"][k]), (name, stage, mode, k)
        for k, g in a["grads"].items():
            assert torch.equal(g, b["grads"][k]), (name, stage, mode, k)
        for k, v in a["buffers"].items():
            assert torch.equal(v, b["buffers"][k]), (name, stage, mode, k)


def test_refusals(dev):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    for stage in ("pre", "post"):
        mod = _hip_processor("c", "eval", dev)
        t = {k: v.to(dev).requires_grad_() for k, v in Q.case_tensors("c", stage).items()}
        args = [t[k] for k in Q.INPUTS[stage]]
        outs = train_fn.deeppruner_processor(mod, stage, *args)
        with pytest.raises(NotImplementedError, match="double backward"):
            torch.autograd.grad(sum(o.sum() for o in outs), t["left"], create_graph=True)
        with pytest.raises(NotImplementedError, match="no backward"):
            mod(stage, *args)                                    # the module's own forward stays inference only
        with pytest.raises(NotImplementedError, match="no backward"):
            mod(stage, *[a.detach() for a in args])              # eval(), but grad mode on and the parameters require grad
        with torch.no_grad():
            again = train_fn.deeppruner_processor(mod, stage, *[a.detach() for a in args])
        assert all(not o.requires_grad and torch.equal(o, p) for o, p in zip(again, outs))     # under no_grad: the same launches

