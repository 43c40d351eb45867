"""Record tests/golden/deeppruner_aggregator_bwd.npz from the REAL reference DeepPrunerAggregator and HWHourglass
(dmb/modeling/stereo/cost_processors): forward + backward on the CPU at 8 threads, in train() and eval(), on the runs of
tests/_hw_bwd_ref.py (``RUNS``; its docstring lists the keys).  The loss is a fixed random projection of the output.

Data only: the loss, the input gradient, per parameter the gradient's sum, its largest magnitude and 64 entries at seeded positions,
the updated running buffers.  Inputs, weights and the projection are regenerated from their seeds, never stored.

The script asserts that autograd through the restatement of tests/_hw_ref.py equals the reference's loss, gradients and buffers bit
for bit: that makes the restatement the yardstick everywhere else.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_deeppruner_aggregator_bwd.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import _hw_bwd_ref as Q  # noqa: E402
from tests import _hw_ref as R  # noqa: E402


def record(out, prefix, name, mode, res):
    """The golden entries of one run (tests/_hw_bwd_ref.py: the module's docstring)"""
    out[prefix + "loss"] = res["loss"].numpy()
    dx = res["dx"]
    if (name, mode) in Q.SAMPLED_DX:
        out[prefix + "dx_stats"] = np.array([dx.double().sum().item(), dx.abs().max().item()])
        out[prefix + "dx_samples"] = dx.flatten()[Q.positions(prefix + "dx", dx.numel(), Q.SAMPLES_DX)].numpy()
    else:
        out[prefix + "dx"] = dx.numpy()
    for k, g in res["grads"].items():
        out[prefix + "p/" + k + "/stats"] = np.array([g.double().sum().item(), g.abs().max().item()])
        out[prefix + "p/" + k + "/samples"] = g.flatten()[Q.positions(prefix + k, g.numel())].numpy()
    if mode == "train":
        for k, v in res["buffers"].items():
            out[prefix + "b/" + k] = v.numpy()


def main():
    import_reference()
    from dmb.modeling.stereo.cost_processors.aggregators.DeepPruner import DeepPrunerAggregator
    from dmb.modeling.stereo.cost_processors.utils.hw_hourglass import HWHourglass

    torch.set_num_threads(8)
    out = {}
    for name, mode in Q.RUNS:
        kind = Q.CASES[name][0]
        ref_mod = (HWHourglass(R.HOURGLASS_IN_PLANES, batch_norm=True) if kind == "hourglass"
                   else DeepPrunerAggregator(R.IN_PLANES, R.HOURGLASS_IN_PLANES, batch_norm=True))
        ref_mod = Q.fill(ref_mod, name).train(mode == "train")
        ref = Q.run(ref_mod, name)
        mine = Q.reference(name, mode, torch.float32)
        assert torch.equal(ref["out"], mine["out"]) and torch.equal(ref["loss"], mine["loss"]), (name, mode)
        assert torch.equal(ref["dx"], mine["dx"]), "restatement's input gradient differs from the reference: %s %s" % (name, mode)
        assert list(ref["grads"]) == list(mine["grads"]) and len(ref["grads"]) + 1 == Q.N_TENSORS[kind]
        for k, g in ref["grads"].items():
            assert torch.equal(g, mine["grads"][k]), "restatement's gradient of %s differs from the reference: %s %s" % (k, name, mode)
        for k, v in ref["buffers"].items():
            assert torch.equal(v, mine["buffers"][k]), (name, mode, k)
        f64 = Q.reference(name, mode, torch.float64)
        n, tight = Q.whole_network_rule(Q.tensors(mine), Q.tensors(f64), Q.tensors(mine), "%s %s: FP32 restatement" % (name, mode))
        worst = max((g.double() - f64["grads"][k]).abs().max().item() / f64["grads"][k].abs().max().item() for k, g in ref["grads"].items())
        print("%s %s %s: restatement == reference (%d tensors); loss %.6g; FP32 vs FP64 gradients: worst %.3g of a tensor's range"
              % (name, mode, Q.CASES[name][1], n, ref["loss"].item(), worst))
        record(out, "%s/%s/" % (name, mode), name, mode, ref)
    path = os.path.join(ROOT, "tests", "golden", "deeppruner_aggregator_bwd.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
