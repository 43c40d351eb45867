"""The backward of DeepPruner's aggregator on the MI355X (layers/train_fn.py: ``hw_hourglass``, ``deeppruner_aggregator`` and the
stride-(1, 2, 2) / 16-channel units on ``ConvUnitFn``).

UNITS -- one unit, or a two-unit chain inside ``carry_scope()``, through ``train_fn.conv_unit`` (the modules' own ``forward`` stays
inference only), against the unit's own torch children on the CPU in FP64 and FP32, with the machinery of tests/test_unit_grads_gpu.py:
the upstream gradient is zero wherever the FP64 pre-activation of a ReLU lies within MARGIN x max of zero, so no ReLU can flip and
EVERY tensor (output, dx, dw, dgamma, dbeta, dres) is held to |hip - fp64| <= 4 |fp32 - fp64| + 2e-6 x range; running buffers within
1e-5 relative; a second pass bit-identical.  The share of upstream elements the margin zeroes is asserted below 1 % per case.
Per (unit, shape): BatchNorm none / batch statistics / running statistics x the gradient carry on / off.

NETWORKS -- the hourglass and the aggregator through the two new functions against autograd through tests/_hw_ref.py
(tests/_hw_bwd_ref.py: cases, loss, rule), in eval() with trainable weights and, at the first shape of each pair, in train().  A ReLU
inside the network may flip, which no mask on the upstream gradient can prevent, so the rule is the whole-network rule of
tests/test_backward_gpu.py: every gradient within 3e-2 of its range, at least 60 % of the tensors within 4 |fp32 - fp64| + 2e-5 x
range.  The recorded gradients of the real reference (tests/golden/deeppruner_aggregator_bwd.npz) are matched under the same rule."""
import os

import numpy as np
import pytest
import torch

from tests import _hw_bwd_ref as Q
from tests.test_deeppruner_aggregator_gpu import _check
from tests.test_unit_grads_gpu import MARGIN, _buffers, _compare, _init, _leaves, _params, _pass, _RefUnit, _Toggles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "deeppruner_aggregator_bwd.npz")
HW = (1, 2, 2)

# name -> (units as (Ci, Co, stride, transposed), input channels).  Chains: "down_skip" = conv (1, 2, 2) then stride 1 with the skip
# after the ReLU (conv*_a, conv*_b of the hourglass); "down_up" = conv (1, 2, 2) then the transposed unit with the chain's input as
# its residual (x has two consumers: the carry hands the residual's share to the first unit).
UNITS = {
    "conv_16_32": ([(16, 32, HW, False)], 16), "conv_32_64": ([(32, 64, HW, False)], 32), "conv_64_128": ([(64, 128, HW, False)], 64),
    "s1_32_16": ([(32, 16, 1, False)], 32),
    "deconv_128_64": ([(128, 64, HW, True)], 128), "deconv_64_32": ([(64, 32, HW, True)], 64), "deconv_32_16": ([(32, 16, HW, True)], 32),
    "down_skip": ([(16, 32, HW, False), (32, 32, 1, False)], 16), "down_up": ([(32, 64, HW, False), (64, 32, HW, True)], 32),
    "deconv_residual": ([(64, 32, HW, True)], 64),
}
SHAPES = {"a": (2, 3, 8, 16), "odd": (1, 2, 7, 13), "b": (2, 5, 16, 24)}       # (B, D, H, W)
UNIT_CASES = [(u, s) for u in UNITS for s in SHAPES
              if not (s == "odd" and (any(t for _, _, _, t in UNITS[u][0]) or u == "down_up"))]


def _make_units(name, bn, dev, g):
    from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers import FusedConv3d
    mods = [FusedConv3d(bn != "none", ci, co, 3, s, 1, 1, False, relu=not t, transposed=t, output_padding=(0, 1, 1) if t else 0)
            for ci, co, s, t in UNITS[name][0]]
    _init(mods, g)
    mods = [m.to(dev).train(bn == "train") for m in mods]
    for m in mods:
        for p in m.parameters():
            p.requires_grad_(True)
    return mods


def _call(name):
    """call(mods, t) -> outputs, for the device units (through train_fn.conv_unit) and for _RefUnit alike"""
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn

    def unit(m, x, residual=None, relu=False):
        return m(x, residual=residual, relu=relu) if isinstance(m, _RefUnit) else train_fn.conv_unit(m, x, residual, relu)
    if name == "down_skip":
        def call(m, t):
            a = unit(m[0], t["x"], None, False)     # (no ReLU inside the chain: the upstream mask could not keep it from flipping)
            return [unit(m[1], a, a, "pre")]
    elif name == "down_up":
        def call(m, t):
            return [unit(m[1], unit(m[0], t["x"], None, False), t["x"], False)]
    elif name == "deconv_residual":
        def call(m, t):
            return [unit(m[0], t["x"], t["r"], False)]
    else:
        def call(m, t):
            return [unit(m[0], t["x"], None, not m[0].transposed if not isinstance(m[0], _RefUnit) else m[0].relu)]
    return call


def _ref(m, dtype):
    r = _RefUnit(m, dtype)
    r.relu = not m.transposed
    return r


def _check_units(name, mods, t64, carry, dev, g):
    """tests/test_unit_grads_gpu.py: _check_case, with the share of the margin asserted"""
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    call, fails = _call(name), []
    ref64, ref32 = [_ref(m, torch.float64) for m in mods], [_ref(m, torch.float32) for m in mods]
    saved = [{k: v.detach().clone() for k, v in _buffers(m).items()} for m in mods]
    t_64 = _leaves(t64, torch.float64, "cpu")
    outs64 = call(ref64, t_64)
    gs, zeroed, total = [], 0, 0
    for o, pre in zip(outs64, [ref64[-1].pre]):
        gi = torch.randn(o.shape, generator=g, dtype=torch.float64)
        if pre is not None:
            mask = pre.detach().abs() < MARGIN * pre.detach().abs().max()
            gi[mask] = 0.0
            zeroed += int(mask.sum())
        total += gi.numel()
        gs.append(gi)
    assert zeroed < 0.01 * total, "the margin zeroes %d of %d upstream elements" % (zeroed, total)
    torch.autograd.backward(outs64, gs)
    grads64 = {("in", k): v.grad for k, v in t_64.items()}
    for i, m in enumerate(ref64):
        for n, p in _params(m).items():
            grads64[(i, n)] = p.grad
    outs32, grads32 = _pass(ref32, call, _leaves(t64, torch.float32, "cpu"), gs)
    runs = []
    for rep in range(2):
        if rep:
            with torch.no_grad():
                for m, s in zip(mods, saved):
                    for k, v in _buffers(m).items():
                        if not torch.equal(v, s[k].to(v.device)):
                            v.copy_(s[k])
        with _Toggles(dict(split_k=True, carry=carry, pack_group=True, epilogue=False)):
            outs, grads = _pass(mods, call, _leaves(t64, torch.float32, dev), gs, train_fn.carry_scope)
        torch.cuda.synchronize()
        bufs = [{k: v.detach().cpu().clone() for k, v in _buffers(m).items()} for m in mods]
        runs.append(([o.detach().cpu() for o in outs], {k: (v.detach().cpu() if v is not None else None) for k, v in grads.items()}, bufs))
        if rep == 0 and type(outs[0].grad_fn).__name__ != "ConvUnitFnBackward":
            fails.append("output made by %s" % type(outs[0].grad_fn).__name__)
    (outs, grads, bufs), (outs2, grads2, _) = runs
    gmax = max([v.detach().abs().max().item() for v in grads64.values() if v is not None and v.numel()] + [0.0])
    for i, (o, o64, o32) in enumerate(zip(outs, outs64, outs32)):
        _compare("output %d" % i, o, o64, o32, 0.0, fails)
    assert set(grads) == set(grads64)
    for k in grads64:
        _compare("d%s" % (k,), grads.get(k), grads64[k], grads32[k], 1e-6 * gmax, fails)
    for i, (m64, b) in enumerate(zip(ref64, bufs)):
        for k, v64 in _buffers(m64).items():
            if v64.dtype == torch.int64:
                if not torch.equal(b[k], v64):
                    fails.append("unit %d %s: %s != %s" % (i, k, b[k].tolist(), v64.tolist()))
            elif not (b[k].double() - v64).abs().max().item() <= 1e-5 * max(v64.abs().max().item(), 1e-2):
                fails.append("unit %d %s: error %.3e" % (i, k, (b[k].double() - v64).abs().max().item()))
    if not all(torch.equal(a, b) for a, b in zip(outs, outs2)):
        fails.append("second pass: output differs")
    for k, v in grads.items():
        if (v is None) != (grads2[k] is None) or (v is not None and not torch.equal(v, grads2[k])):
            fails.append("second pass: d%s not bit-identical" % (k,))
    return fails


@pytest.mark.parametrize("name,shape", UNIT_CASES, ids=["%s-%s" % c for c in UNIT_CASES])
def test_units_forward_and_backward_against_fp64(dev, name, shape):
    B, D, H, W = SHAPES[shape]
    units, Ci = UNITS[name]
    failures = []
    for n, (bn, carry) in enumerate((b, c) for b in ("none", "train", "eval") for c in (True, False)):
        g = torch.Generator().manual_seed(81000 + 100 * list(UNITS).index(name) + 10 * list(SHAPES).index(shape) + n)
        mods = _make_units(name, bn, dev, g)
        t64 = {"x": torch.randn((B, Ci, D, H, W), generator=g, dtype=torch.float64)}
        if name == "deconv_residual":
            t64["r"] = torch.randn((B, units[0][1], D, 2 * H, 2 * W), generator=g, dtype=torch.float64)
        failures += ["%s carry %s: %s" % (bn, carry, f) for f in _check_units(name, mods, t64, carry, dev, g)]
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------- networks
def _hip_module(name, mode, dev):
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.aggregators import DeepPrunerAggregator
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils import HWHourglass
    from tests import _hw_ref as R
    m = HWHourglass(R.HOURGLASS_IN_PLANES) if Q.CASES[name][0] == "hourglass" else DeepPrunerAggregator(R.IN_PLANES, R.HOURGLASS_IN_PLANES)
    return Q.fill(m, name).to(dev).train(mode == "train")


def _forward(name):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    return (lambda m, x: train_fn.hw_hourglass(m, x)) if Q.CASES[name][0] == "hourglass" else train_fn.deeppruner_aggregator


@pytest.mark.parametrize("name,mode", Q.RUNS, ids=["%s-%s" % r for r in Q.RUNS])
def test_networks_against_autograd_through_the_restatement(dev, name, mode):
    kind = Q.CASES[name][0]
    mod = _hip_module(name, mode, dev)
    before = {k: v.detach().clone() for k, v in mod.named_buffers()}
    res = Q.run(mod, name, forward=_forward(name), device=dev)
    torch.cuda.synchronize()
    r64, r32 = Q.reference(name, mode, torch.float64), Q.reference(name, mode, torch.float32)
    # the output: the aggregator's forward contract (tests/test_deeppruner_aggregator_gpu.py), also for the modules' own eval forward
    _check(res["out"], r32["out"], r64["out"], "%s %s output" % (name, mode))
    # the loss, a sum: 4x the FP32 restatement's own error plus 2e-6 of the sum of its terms' magnitudes
    mass = (r64["out"] * Q.projection(name, r64["out"].shape).double()).abs().sum().item()
    assert abs(res["loss"].item() - r64["loss"].item()) <= 4 * abs(r32["loss"].item() - r64["loss"].item()) + 2e-6 * mass
    n, tight = Q.whole_network_rule(Q.tensors(res), Q.tensors(r64), Q.tensors(r32), "%s %s" % (name, mode))
    print("%s %s: %d of %d gradients within the tight bound" % (name, mode, tight, n))
    assert n == Q.N_TENSORS[kind]
    for k, v in mod.named_buffers():
        if mode == "eval":
            assert torch.equal(v, before[k]), k
        else:
            want = r64["buffers"][k]
            assert (v.cpu().double() - want.double()).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item()), k
    # the recorded gradients of the real reference, under the same rule (the recording stands in for the FP32 evaluation)
    z = np.load(GOLDEN)
    prefix = "%s/%s/" % (name, mode)
    got, ref, gold = {}, {}, {}
    for k, t in Q.tensors(res).items():
        if k == "input":
            full = (name, mode) not in Q.SAMPLED_DX
            pos = None if full else Q.positions(prefix + "dx", t.numel(), Q.SAMPLES_DX)
            gold[k] = torch.from_numpy(z[prefix + ("dx" if full else "dx_samples")]).flatten()
        else:
            pos = Q.positions(prefix + k, t.numel())
            gold[k] = torch.from_numpy(z[prefix + "p/" + k + "/samples"])
        r = Q.tensors(r64)[k].flatten()
        # (range and error of a sampled tensor: of the samples plus the recorded largest magnitude's place in the rule's range)
        got[k], ref[k] = (t.detach().cpu().flatten(), r) if pos is None else (t.detach().cpu().flatten()[pos], r[pos])
    assert Q.whole_network_rule(got, ref, gold, "%s %s against the recording" % (name, mode))[0] == Q.N_TENSORS[kind]
    if mode == "eval":
        with torch.no_grad():
            x = Q.case_input(name).to(dev)
            own = mod(x)
            own = own[0] if isinstance(own, list) else own
            again = _forward(name)(mod, x)
            again = again[0] if isinstance(again, list) else again
        _check(own, r32["out"], r64["out"], "%s: the module's eval forward" % name)
        assert not again.requires_grad and torch.equal(again, res["out"])       # the function under no_grad: the same launches


def test_a_second_forward_and_backward_is_bit_identical(dev):
    for name, mode in (("hg_b", "eval"), ("agg_b", "eval"), ("hg_a", "train")):
        runs = []
        for _ in range(2):
            mod = _hip_module(name, mode, dev)          # (train(): the running buffers start from the same values)
            runs.append(Q.run(mod, name, forward=_forward(name), device=dev))
        a, b = runs
        assert torch.equal(a["out"], b["out"]) and torch.equal(a["dx"], b["dx"]), (name, mode)
        for k, g in a["grads"].items():
            assert torch.equal(g, b["grads"][k]), (name, mode, k)
        for k, v in a["buffers"].items():
            assert torch.equal(v, b["buffers"][k]), (name, mode, k)


def test_refusals(dev):
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils import HWHourglass
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    for name in ("hg_b", "agg_b"):
        mod = _hip_module(name, "eval", dev)
        x = Q.case_input(name).to(dev).requires_grad_()
        out = _forward(name)(mod, x)
        out = out[0] if isinstance(out, list) else out
        with pytest.raises(NotImplementedError, match="double backward"):
            torch.autograd.grad(out.sum(), x, create_graph=True)
        with pytest.raises(NotImplementedError, match="no backward"):
            mod(x)                                          # the modules' own forward stays inference only
        with pytest.raises(NotImplementedError, match="no backward"):
            mod(x.detach())                                 # eval(), but grad mode on and the parameters require grad
    x = torch.zeros((1, 16, 2, 8, 8), device=dev)
    with pytest.raises(NotImplementedError, match="no backward"):
        HWHourglass(16).to(dev).train()(x)
    with pytest.raises(ValueError, match="multiples of 8"):
        train_fn.hw_hourglass(HWHourglass(16).to(dev), torch.zeros((1, 16, 2, 12, 8), device=dev))
