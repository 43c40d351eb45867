"""The backward of DeepPruner's refinement on the MI355X (layers/train_fn.py: ``RefineHeadFn`` / ``refinement_head`` and
``deeppruner_refinement``).

HEAD -- ``refinement_head`` at the six shapes of tests/test_wgrad_c1_2d_gpu.py against the reference composition
(tests/_deeppruner_features_ref.py: ``refine_tail``) on the CPU in FP64 and FP32.  The inputs are built so that the ReLU cannot
flip: wherever the FP64 pre-activation conv(x) + init lies within MARGIN x max of zero (MARGIN of tests/test_unit_grads_gpu.py),
``init`` is moved away from zero by twice that margin, so no element is left out and EVERY tensor (output, dx, d_init, dw) is held
to |hip - fp64| <= 4 |fp32 - fp64| + 2e-6 x range.  Every shape with more than 16 pixels has 30 - 70 % positive pre-activations.
The forward is ``torch.equal`` to ``ops_deeppruner.refine_head_up2`` and a second pass is bit-identical.

CASCADE -- ``deeppruner_refinement`` on the three recorded cases (tests/_deeppruner_refinement_bwd_ref.py: runs, loss), in eval()
with trainable weights and, on the two-stage case, in train(), against autograd through the restatement in FP64 and FP32.  A ReLU
inside the network may flip, so the rule is the whole-network rule of tests/test_backward_gpu.py -- every gradient within 3e-2 of
its range, at least 60 % of the tensors within 4 |fp32 - fp64| + 2e-5 x range -- for every input's gradient and every
parameter's; the recorded gradients of the real reference (tests/golden/deeppruner_refinement_bwd.npz) are matched under the same
rule; the returned maps are held to the forward contract of tests/test_deeppruner_features_gpu.py (``_check``); running buffers
within 1e-5 relative; ``grad_fn`` names prove that the path was taken."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _deeppruner_features_ref as R
from tests import _deeppruner_refinement_bwd_ref as Q
from tests._hw_bwd_ref import whole_network_rule
from tests.test_backward_gpu import _close
from tests.test_deeppruner_features_gpu import _check
from tests.test_unit_grads_gpu import MARGIN
from tests.test_wgrad_c1_2d_gpu import CASES as HEAD_SHAPES

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------- head
def _tail(x, w, init, gy, dtype):
    x, w, init = (t.detach().clone().to(dtype).requires_grad_() for t in (x, w, init))     # (the cached operands stay plain)
    y = R.refine_tail(x, w, init)
    y.backward(gy.to(dtype))
    return dict(output=y.detach(), dx=x.grad, d_init=init.grad, dw=w.grad)


@functools.lru_cache(maxsize=None)
def _head_data(name):
    """Operands (CPU, FP32), the upstream gradient and the FP64 / FP32 results of a shape: computed once, never modified."""
    (B, Ci, H, W), _ = HEAD_SHAPES[name]
    g = torch.Generator().manual_seed(9840 + list(HEAD_SHAPES).index(name))     # (at this base the single pixel of one_pixel is positive)
    x = torch.randn((B, Ci, H, W), generator=g)
    w = torch.randn((1, Ci, 3, 3), generator=g) * (1.0 / (Ci * 9)) ** 0.5
    init = torch.randn((B, 1, H, W), generator=g)
    pre = F.conv2d(x.double(), w.double(), padding=1) + init.double()
    margin = MARGIN * pre.abs().max().item()
    near = pre.abs() < margin
    init = torch.where(near, init + torch.where(pre < 0, -2 * margin, 2 * margin).float(), init)
    pre = F.conv2d(x.double(), w.double(), padding=1) + init.double()
    assert not bool((pre.abs() < margin).any()), "%s: a pre-activation is still within the margin of zero" % name
    positive = (pre > 0).double().mean().item()
    assert positive > 0, "%s: the ReLU clamps every element, so no gradient would be compared" % name
    if B * H * W > 16:
        assert 0.3 <= positive <= 0.7, "%s: %.0f %% positive pre-activations" % (name, 100 * positive)
    gy = torch.randn((B, 1, 2 * H, 2 * W), generator=g)
    return x, w, init, gy, _tail(x, w, init, gy, torch.float64), _tail(x, w, init, gy, torch.float32)


class _Block:
    """What ``refinement_head`` reads of a RefinementHeand"""

    def __init__(self, w):
        self.classify = torch.nn.Conv2d(w.shape[1], 1, 3, padding=1, bias=False).to(w.device)
        with torch.no_grad():
            self.classify.weight.copy_(w)


def _head_pass(x, w, init, gy, dev):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    block = _Block(w.to(dev))
    xd, idev = x.to(dev).requires_grad_(), init.to(dev).requires_grad_()
    y = train_fn.refinement_head(block, idev, xd)
    y.backward(gy.to(dev))
    torch.cuda.synchronize()
    return y, dict(output=y.detach(), dx=xd.grad, d_init=idev.grad, dw=block.classify.weight.grad)


@pytest.mark.parametrize("name", list(HEAD_SHAPES))
def test_refinement_head_forward_and_backward_against_fp64(dev, name):
    from densematchingbenchmark_amd import ops, ops_deeppruner
    x, w, init, gy, r64, r32 = _head_data(name)
    assert ops.conv_wgrad_plan(4, x.to(dev), init.to(dev), 3, 1)[0] == 0x700
    y, got = _head_pass(x, w, init, gy, dev)
    assert type(y.grad_fn).__name__ == "RefineHeadFnBackward"
    assert torch.equal(got["output"], ops_deeppruner.refine_head_up2(x.to(dev), w.to(dev), init.to(dev))), "the fused head's bits"
    for k in ("output", "dx", "d_init", "dw"):
        assert got[k] is not None and got[k].shape == r64[k].shape, k
        e, own, rng = ((got[k].cpu().double() - r64[k]).abs().max().item(), (r32[k].double() - r64[k]).abs().max().item(),
                       r64[k].abs().max().item())
        print("%s %s: error %.3e, fp32 error %.3e, range %.3e" % (name, k, e, own, rng))
        _close(got[k].cpu(), r64[k], r32[k], "%s %s" % (name, k))
    _, again = _head_pass(x, w, init, gy, dev)
    for k, v in got.items():
        assert torch.equal(v, again[k]), "%s: second pass, %s not bit-identical" % (name, k)


def test_refinement_head_gradients_only_where_asked(dev):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    x, w, init, gy, r64, r32 = _head_data("odd_width")
    block = _Block(w.to(dev))
    idev = init.to(dev).requires_grad_()
    block.classify.weight.requires_grad_(False)
    y = train_fn.refinement_head(block, idev, x.to(dev))
    y.backward(gy.to(dev))
    assert block.classify.weight.grad is None
    _close(idev.grad.cpu(), r64["d_init"], r32["d_init"], "d_init alone")
    with pytest.raises(NotImplementedError, match="double backward"):
        xd = x.to(dev).requires_grad_()
        torch.autograd.grad(train_fn.refinement_head(block, idev, xd).sum(), xd, create_graph=True)


# ------------------------------------------------------------------------------------------------------------- cascade
def _hip_refinement(name, mode, dev):
    from densematchingbenchmark_amd.modeling.stereo.disp_refinement import DeepPrunerRefinement
    (planes, num, _, _), _ = R.REFINE_CASES[name]
    return Q.fill(DeepPrunerRefinement(list(planes), True, num)).to(dev).train(mode == "train")


def _hip_run(name, mode, dev, mod=None):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    mod = mod if mod is not None else _hip_refinement(name, mode, dev)
    res = Q.run(mod, name, forward=train_fn.deeppruner_refinement, device=dev)
    torch.cuda.synchronize()
    return mod, res


@pytest.mark.parametrize("name,mode", Q.GPU_RUNS, ids=["%s-%s" % r for r in Q.GPU_RUNS])
def test_refinement_against_autograd_through_the_restatement(dev, name, mode):
    what = "%s %s" % (name, mode)
    num = R.REFINE_CASES[name][0][1]
    mod = _hip_refinement(name, mode, dev)
    before = {k: v.detach().clone() for k, v in mod.named_buffers()}
    mod, res = _hip_run(name, mode, dev, mod)
    r64, r32 = Q.reference(name, mode, torch.float64), Q.reference(name, mode, torch.float32)
    # the path: one RefineStageFn per stage; the incoming map is returned as it came, last
    assert res["grad_fns"] == ["RefineStageFnBackward"] * num + ["NoneType"], res["grad_fns"]
    assert len(res["outs"]) == num + 1 and torch.equal(res["outs"][-1].cpu(), Q.case_tensors(name)["disp"])
    for i, (o, o32, o64) in enumerate(zip(res["outs"][:num], r32["outs"], r64["outs"])):      # the forward contract of the eval path
        _check(o, o32, o64, "%s map %d" % (what, i))
    # the loss, a sum: 4x the FP32 restatement's own error plus 2e-6 of the sum of its terms' magnitudes
    mass = sum((o * p.double()).abs().sum().item() for o, p in zip(r64["outs"], Q.projections(name, r64["outs"])))
    print("%s loss: error %.3e, fp32 error %.3e, mass %.3e" % (what, abs(res["loss"].item() - r64["loss"].item()),
                                                             abs(r32["loss"].item() - r64["loss"].item()), mass))
    assert abs(res["loss"].item() - r64["loss"].item()) <= 4 * abs(r32["loss"].item() - r64["loss"].item()) + 2e-6 * mass
    got = Q.tensors(res)
    assert len(res["grads"]) == 19 * num and sorted(res["grads"]) == sorted(r64["grads"])
    n, tight = whole_network_rule(got, Q.tensors(r64), Q.tensors(r32), what)
    print("%s: %d of %d gradients within the tight bound" % (what, tight, n))
    assert n == 1 + num + 19 * num
    # the recorded gradients of the real reference under the same rule (the recording stands in for FP32)
    z = np.load(Q.GOLDEN)
    prefix = "%s/%s/" % (name, mode)
    gold = {"in/disp": torch.from_numpy(z[prefix + "in/disp"])}
    live, ref = {"in/disp": res["inputs"]["disp"]}, {"in/disp": r64["inputs"]["disp"]}
    fms = {k: g for k, g in res["inputs"].items() if k != "disp"}
    shapes = {k: tuple(g.shape) for k, g in list(fms.items()) + list(res["grads"].items())}
    for part, grads, n_s in (("in", fms, Q.IN_SAMPLES), ("p", res["grads"], Q.SAMPLES)):
        src = r64["inputs"] if part == "in" else r64["grads"]
        tag = "in/" if part == "in" else ""
        for k, v in Q.recorded(z, prefix, part, shapes, n_s).items():
            gold[tag + k] = v
        for k, v in Q.sampled(prefix, grads, n_s).items():
            live[tag + k] = v
        for k, v in Q.sampled(prefix, {k: src[k] for k in grads}, n_s).items():
            ref[tag + k] = v
    whole_network_rule(live, ref, gold, what + " against the recording")
    for k, v in mod.named_buffers():
        if mode == "eval":
            assert torch.equal(v, before[k]), k
        else:
            want = r64["buffers"][k]
            assert (v.cpu().double() - want.double()).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item()), k
            assert not torch.equal(v, before[k]) or v.numel() == 0, k


def test_a_second_pass_is_bit_identical(dev):
    for name, mode in (("rodd", "eval"), ("r8x", "train")):
        a, b = (_hip_run(name, mode, dev)[1] for _ in range(2))     # (train(): the buffers start from the same values)
        assert all(torch.equal(x, y) for x, y in zip(a["outs"], b["outs"])), (name, mode)
        for k, g in Q.tensors(a).items():
            assert torch.equal(g, Q.tensors(b)[k]), (name, mode, k)
        for k, v in a["buffers"].items():
            assert torch.equal(v, b["buffers"][k]), (name, mode, k)


def test_saved_tensor_rules_of_the_one_node_stage(dev):
    """RefineStageFn keeps its units' tensors on plain context objects (train_fn._PlainCtx).  Pinned here: a parameter modified in
    place between forward and backward is refused, as autograd refuses it; a second backward over the same graph runs without
    ``retain_graph`` and gives the same bits (the tensors live as long as the node)."""
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    mod = _hip_refinement("rodd", "eval", dev)
    t = {k: v.to(dev).requires_grad_() for k, v in Q.case_tensors("rodd").items()}
    leaves = [t["disp"], t["fms0"]] + list(mod.parameters())
    out = train_fn.deeppruner_refinement(mod, [t["disp"]], [t["fms0"]])[0]
    up = torch.ones_like(out)
    first = torch.autograd.grad(out, leaves, up)
    second = torch.autograd.grad(out, leaves, up)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for victim in (mod.refine_blocks[0].conv[2][0].weight, mod.refine_blocks[0].classify.weight):
        out = train_fn.deeppruner_refinement(mod, [t["disp"]], [t["fms0"]])[0]
        with torch.no_grad():
            victim.mul_(1.0)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            torch.autograd.grad(out, leaves, up)


def test_refusals_and_the_inference_path(dev):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    mod = _hip_refinement("rodd", "eval", dev)
    t = {k: v.to(dev).requires_grad_() for k, v in Q.case_tensors("rodd").items()}
    outs = train_fn.deeppruner_refinement(mod, [t["disp"]], [t["fms0"]])
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(outs[0].sum(), t["fms0"], create_graph=True)
    with pytest.raises(NotImplementedError, match="the fused refinement head has none"):
        mod([t["disp"]], [t["fms0"]])                        # the module's own forward stays inference only
    with torch.no_grad():
        fused = mod([t["disp"].detach()], [t["fms0"].detach()])
    # eval(): the six layers run the fused conv2d kernel there and separate launches here, so the maps agree to rounding, not in bits
    assert len(fused) == len(outs) == 2
    rng = fused[0].abs().max().item()
    assert (fused[0] - outs[0].detach()).abs().max().item() <= 1e-4 * rng
