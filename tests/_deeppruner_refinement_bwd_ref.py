"""Yardstick of the DeepPruner refinement BACKWARD tests: forward + backward of the restatement of
tests/_deeppruner_features_ref.py (``DeepPrunerRefinement`` in plain torch.nn, any dtype) on its seeded weights and the inputs of
its three ``REFINE_CASES``, with a fixed seeded projection of the returned maps as the loss.  Shared by the host test, the GPU test
and scripts/gen_golden_deeppruner_refinement_bwd.py, which records the REAL reference's results in
tests/golden/deeppruner_refinement_bwd.npz after asserting that this restatement equals them bit for bit on the CPU.

A RUN is (case, mode): case r4x (one stage) | r8x (two stages) | rodd (odd sizes below one tile); mode "eval" = eval() with
trainable weights (running statistics, buffers untouched) or "train" = train() (batch statistics, buffers updated).

INPUTS of a run: ``disp`` (the incoming disparity, which has three consumers: the first guide's last channel, the first head's
``init`` and its own place in the returned list) and ``fms0`` (, ``fms1``), the guide features.  The loss covers EVERY returned map,
the incoming one included.  Nothing between the inputs and the loss is discontinuous but the ReLUs, so the FP64 restatement is the
yardstick of every gradient.

The golden file holds, per run ``<case>/<mode>/``: ``loss``; ``in/disp`` (in full); ``in/names``, ``in/stats``, ``in/samples`` (the
feature maps' gradients: sum, largest magnitude and IN_SAMPLES entries at seeded positions); ``p/names``, ``p/stats``,
``p/samples`` (the parameters' likewise, SAMPLES entries, in ``named_parameters`` order); in train mode ``b/names`` and the updated
running buffers ``b/<index>``."""
import os

import numpy as np
import torch

from tests import _deeppruner_features_ref as R
from tests import _deeppruner_processor_bwd_ref as Q

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deeppruner_refinement_bwd.npz")
MODES = ("eval", "train")
RUNS = [(c, m) for c in R.REFINE_CASES for m in MODES]
GPU_RUNS = [(c, m) for c, m in RUNS if m == "eval" or c == "r8x"]      # train() on the two-stage case only: the GPU suite stays quick
SAMPLES, IN_SAMPLES = Q.SAMPLES, 4096


def inputs_of(name):
    """The input names of a case, in order"""
    return ("disp",) + tuple("fms%d" % i for i in range(R.REFINE_CASES[name][0][1]))


def case_tensors(name, dtype=torch.float32):
    """{input name: CPU tensor} of a case"""
    disps, fms = R.refine_inputs(name, dtype)
    return dict([("disp", disps[0])] + [("fms%d" % i, f) for i, f in enumerate(fms)])


def projections(name, outs):
    """The fixed random tensors whose inner products with the returned maps add up to the loss"""
    g = torch.Generator().manual_seed(R.REFINE_CASES[name][1] + 900)
    return [torch.randn(tuple(o.shape), generator=g) for o in outs]


def loss_of(name, outs):
    outs = list(outs)
    return sum((o * p.to(device=o.device, dtype=o.dtype)).sum() for o, p in zip(outs, projections(name, outs)))


def fill(module):
    """Seeded weights for any module with the reference's keys (restatement, reference, HIP module)"""
    return R.seeded_state(module, R.WEIGHT_SEED)


def restatement(name, mode, dtype=torch.float32):
    return R.refinement(name, dtype).train(mode == "train")


def run(module, name, forward=None, device="cpu", dtype=torch.float32):
    """Forward + backward of ``module`` from the case's inputs -> dict(outs, loss, inputs {name: gradient}, grads {parameter:
    gradient}, buffers).  ``forward(module, disps, fms)``: default the module's own call."""
    leaves = {k: v.to(device).requires_grad_() for k, v in case_tensors(name, dtype).items()}
    for p in module.parameters():
        p.grad = None
    disps, fms = [leaves["disp"]], [leaves[k] for k in inputs_of(name)[1:]]
    outs = list(forward(module, disps, fms) if forward is not None else module(disps, fms))
    loss = loss_of(name, outs)
    loss.backward()
    grads = {k: p.grad for k, p in module.named_parameters() if p.grad is not None}
    return dict(outs=[o.detach() for o in outs], loss=loss.detach(), inputs={k: v.grad for k, v in leaves.items()}, grads=grads,
                buffers={k: v.detach().clone() for k, v in module.named_buffers()}, grad_fns=[type(o.grad_fn).__name__ for o in outs])


_cache = {}


def reference(name, mode, dtype):
    """The restatement's run on the CPU in ``dtype``: computed once, shared, never modified."""
    key = (name, mode, dtype)
    if key not in _cache:
        _cache[key] = run(restatement(name, mode, dtype), name, dtype=dtype)
    return _cache[key]


def tensors(res):
    """{name: tensor} of a run's compared gradients: every input's and every parameter's"""
    d = {"in/" + k: g for k, g in res["inputs"].items()}
    d.update(res["grads"])
    return d


def packed(prefix, grads, n=SAMPLES):
    """(names, stats [k, 2], samples [k, n]) of gradients, as the golden file holds them"""
    names = list(grads)
    stats = np.array([[g.double().sum().item(), g.abs().max().item()] for g in grads.values()], dtype=np.float64)
    samples = np.zeros((len(names), n), dtype=np.float32)
    for i, (k, g) in enumerate(grads.items()):
        v = g.detach().cpu().flatten()[Q.positions(prefix + k, g.numel(), n)].numpy()
        samples[i, :v.size] = v
    return np.array(names), stats, samples


def sampled(prefix, grads, n=SAMPLES):
    """{name: the sampled entries of its gradient} (CPU, flat), at the golden file's positions"""
    return {k: g.detach().cpu().flatten()[Q.positions(prefix + k, g.numel(), n)] for k, g in grads.items()}


def recorded(z, prefix, what, shapes, n):
    """{name: the recorded samples} of ``<prefix><what>/`` cut to each tensor's size"""
    names = [str(k) for k in z[prefix + what + "/names"]]
    return {k: torch.from_numpy(z[prefix + what + "/samples"][i][:min(n, int(np.prod(shapes[k])))]) for i, k in enumerate(names)}
