"""Yardstick of the DeepPruner cost-processor BACKWARD tests: forward + backward of the restatement of
tests/_deeppruner_processor_ref.py (plain torch.nn, any dtype) on its seeded weights and case inputs, with a fixed seeded projection
of the outputs as the loss.  Shared by the host test, the GPU test and scripts/gen_golden_deeppruner_processor_bwd.py, which records
the REAL reference's results in tests/golden/deeppruner_processor_bwd.npz after asserting that this restatement equals them bit for
bit on the CPU.

A RUN is (case, stage, mode): case a | b | c of ``_deeppruner_processor_ref.CASES``; stage "pre" (volume, range predictor: four
maps) or "post" (volume with the two range feature maps, aggregator, soft arg-min, up-sampling, two 5x5 convolutions: two maps);
mode "eval" = eval() with trainable weights (running statistics, buffers untouched) or "train" = train() (batch statistics, buffers
updated).  The post stage is fed the FP32 pre-stage feature maps of tests/golden/deeppruner_processor.npz (the eval forward) as two
more inputs that want a gradient.

INPUTS of a run: left, right, sample (+ min_feature, max_feature).  ``run`` returns their gradients, the gradient of the raw volume
(where the caller can reach it) and every parameter's that the stage uses.

The FP64 yardstick starts AFTER the volume, as in the forward tests: the FP32 raw volume cast to double is its leaf (an FP64 sampler
would flip ``T > 0`` where T ~ 0), so it covers d raw_cost and the parameters; the inputs' gradients are held to the FP32 restatement
and to the recording.

The golden file holds, per run ``<case>/<stage>/<mode>/``: ``loss``; ``in/<input>`` (the input gradients in full); ``p/names``,
``p/stats`` [n, 2] (sum, largest magnitude) and ``p/samples`` [n, SAMPLES] (entries at seeded positions, all of a smaller tensor,
zero-padded) over the parameters with a gradient, in ``named_parameters`` order; in train mode ``b/names`` and the updated running
buffers of the stage's modules, ``b/<index>``."""
import os
import zlib

import numpy as np
import torch

from tests import _deeppruner_processor_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deeppruner_processor_bwd.npz")
STAGES, MODES = ("pre", "post"), ("eval", "train")
RUNS = [(c, s, m) for c in R.CASES for s in STAGES for m in MODES]
GPU_RUNS = [(c, s, m) for c, s, m in RUNS if m == "eval" or c == "a"]      # train() on case a only: the GPU suite stays quick
SAMPLES = 64
INPUTS = {"pre": ("left", "right", "sample"), "post": ("left", "right", "sample", "min_feature", "max_feature")}


def case_tensors(name, stage):
    """{input name: FP32 CPU tensor} of a run"""
    left, right, pre, post = R.case_inputs(name)
    if stage == "pre":
        return dict(left=left, right=right, sample=pre)
    z = R.recording()
    fmin, fmax = (torch.from_numpy(z["%s/pre/%s" % (name, n)]).clone() for n in ("min_feature", "max_feature"))
    return dict(left=left, right=right, sample=post, min_feature=fmin, max_feature=fmax)


def projections(name, stage, outs):
    """The fixed random tensors whose inner products with the outputs add up to the loss"""
    g = torch.Generator().manual_seed(R.CASES[name][1] + (700 if stage == "pre" else 800))
    return [torch.randn(tuple(o.shape), generator=g) for o in outs]


def loss_of(name, stage, outs):
    outs = list(outs)
    return sum((o * p.to(device=o.device, dtype=o.dtype)).sum() for o, p in zip(outs, projections(name, stage, outs)))


def fill(module):
    """Seeded weights for any module with the reference's keys (restatement, reference, HIP module)"""
    return R.seeded_state(module, R.WEIGHT_SEED)


def restatement(name, mode, dtype=torch.float32):
    return R.processor(name, dtype).train(mode == "train")


def positions(key, numel, n=SAMPLES):
    """Seeded flat positions into a tensor of ``numel`` entries (all of them when it has no more than ``n``)"""
    if numel <= n:
        return torch.arange(numel)
    return torch.randint(numel, (n,), generator=torch.Generator().manual_seed(zlib.crc32(key.encode()) & 0x7fffffff))


def _collect(module, leaves, outs, loss, raw):
    grads = {k: p.grad for k, p in module.named_parameters() if p.grad is not None}
    return dict(outs=[o.detach() for o in outs], loss=loss.detach(), inputs={k: v.grad for k, v in leaves.items()},
                draw=None if raw is None else raw.grad, grads=grads, buffers={k: v.detach().clone() for k, v in module.named_buffers()})


def run(module, name, stage, forward=None, device="cpu"):
    """Forward + backward of an FP32 ``module`` from the case's inputs -> dict(outs, loss, inputs {name: gradient}, draw, grads
    {parameter: gradient}, buffers).  ``forward(module, stage, **inputs)``: default the module's own call.  ``draw`` is the raw
    volume's gradient where ``forward`` is None and the module is the restatement (``from_volume``), else None."""
    leaves = {k: v.to(device).requires_grad_() for k, v in case_tensors(name, stage).items()}
    for p in module.parameters():
        p.grad = None
    raw = None
    args = [leaves[k] for k in INPUTS[stage]]
    if forward is not None:
        outs = forward(module, stage, *args)
    elif hasattr(module, "from_volume"):
        raw = R.raw_volume(*args)
        raw.retain_grad()
        outs = module.from_volume(stage, raw, leaves["sample"])
    else:
        outs = module(stage, *args)
    loss = loss_of(name, stage, outs)
    loss.backward()
    return _collect(module, leaves, list(outs), loss, raw)


def run_fp64(name, stage, mode):
    """The FP64 yardstick: the FP32 raw volume cast to double is the leaf -> dict(outs, loss, draw, grads, buffers)"""
    t = case_tensors(name, stage)
    module = restatement(name, mode, torch.float64)
    with torch.no_grad():
        raw32 = R.raw_volume(*[t[k] for k in INPUTS[stage]])
    raw = raw32.double().requires_grad_()
    outs = module.from_volume(stage, raw, t["sample"].double())
    loss = loss_of(name, stage, outs)
    loss.backward()
    return _collect(module, {}, list(outs), loss, raw)


_cache = {}


def reference(name, stage, mode, dtype):
    """The restatement's run on the CPU in ``dtype`` (FP64: ``run_fp64``): computed once, shared, never modified."""
    key = (name, stage, mode, dtype)
    if key not in _cache:
        _cache[key] = run_fp64(name, stage, mode) if dtype == torch.float64 else run(restatement(name, mode), name, stage)
    return _cache[key]


def zero_by_construction(key, mode):
    """The bias of a 5x5 convolution behind a batch-statistics BatchNorm: the normalisation removes any constant, so its gradient
    is exactly zero.  Autograd leaves rounding noise there (1e-15 in FP64, 1e-5 in FP32), which is no range to measure against."""
    return mode == "train" and key.endswith("feature_conv.0.bias")


def yardstick_tensors(res, mode):
    """{name: tensor} of what the FP64 yardstick covers: the raw volume's gradient and every parameter's, but the biases whose
    gradient is zero by construction (``check_zero_grads`` holds those)"""
    d = {"raw_cost": res["draw"]}
    d.update({k: g for k, g in res["grads"].items() if not zero_by_construction(k, mode)})
    return d


def check_zero_grads(got, ref32, mode, what):
    """A gradient that is zero by construction stays within 4x the FP32 restatement's own rounding noise around zero"""
    n = 0
    for k, g in got.items():
        if zero_by_construction(k, mode):
            assert g.detach().abs().max().item() <= 4 * ref32[k].abs().max().item(), (what, k)
            n += 1
    return n


def whole_network_rule(got, ref64, ref32, what):
    """tests/_hw_bwd_ref.py: every tensor within 3e-2 of its range, at least 60 % of them within 4 |fp32 - fp64| + 2e-5 x range"""
    from tests._hw_bwd_ref import whole_network_rule as rule
    return rule(got, ref64, ref32, what)


def coarse_rule(got, ref, what):
    """The inputs' gradients, which have no FP64 yardstick (module docstring): the whole-network rule's bound for EVERY tensor,
    3e-2 of its range, against the FP32 restatement (a ReLU inside the network may flip; the volume's own adjoint is held to its
    tight rule by the Function's test)."""
    assert sorted(got) == sorted(ref), (what, sorted(set(got) ^ set(ref)))
    for k, r in ref.items():
        assert got[k] is not None, (what, k)
        g, r = got[k].detach().cpu().double(), r.detach().double()
        scale, err = r.abs().max().item(), (g - r).abs().max().item()
        assert err <= 3e-2 * scale, "%s: grad of %s: error %.3e of range %.3e" % (what, k, err, scale)


def packed(prefix, grads):
    """(names, stats [n, 2], samples [n, SAMPLES]) of a run's parameter gradients, as the golden file holds them"""
    names = list(grads)
    stats = np.array([[g.double().sum().item(), g.abs().max().item()] for g in grads.values()], dtype=np.float64)
    samples = np.zeros((len(names), SAMPLES), dtype=np.float32)
    for i, (k, g) in enumerate(grads.items()):
        v = g.detach().cpu().flatten()[positions(prefix + k, g.numel())].numpy()
        samples[i, :v.size] = v
    return np.array(names), stats, samples


def sampled(prefix, grads):
    """{parameter: the sampled entries of its gradient} (CPU, flat), at the golden file's positions"""
    return {k: g.detach().cpu().flatten()[positions(prefix + k, g.numel())] for k, g in grads.items()}
