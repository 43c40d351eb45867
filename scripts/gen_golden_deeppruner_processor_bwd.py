"""Record tests/golden/deeppruner_processor_bwd.npz from the REAL reference ``DeepPrunerProcessor``
(dmb/modeling/stereo/cost_processors/DeepPruner.py): forward + backward on the CPU at 8 threads, for both stages, in train() and
eval(), on the runs of tests/_deeppruner_processor_bwd_ref.py (``RUNS``; its docstring lists the keys).  The loss is a fixed seeded
projection of the outputs.

Data only: the loss, the input gradients, per parameter the gradient's sum, its largest magnitude and 64 entries at seeded positions,
the updated running buffers.  Inputs, weights and the projections are regenerated from their seeds, never stored; the post stage's
two feature maps come from tests/golden/deeppruner_processor.npz.

The script asserts that autograd through the restatement of tests/_deeppruner_processor_ref.py equals the reference's loss,
gradients and buffers bit for bit: that makes the restatement the yardstick everywhere else.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_deeppruner_processor_bwd.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from scripts.gen_golden_deeppruner_processor import _cfg  # noqa: E402
from tests import _deeppruner_processor_bwd_ref as Q  # noqa: E402
from tests import _deeppruner_processor_ref as R  # noqa: E402


def main():
    import_reference()
    from dmb.modeling.stereo.cost_processors.DeepPruner import DeepPrunerProcessor

    torch.set_num_threads(8)
    out = {}
    for name, stage, mode in Q.RUNS:
        (B, C, P, N, H, W), _ = R.CASES[name]
        ref_mod = Q.fill(DeepPrunerProcessor(_cfg(C, P, N))).train(mode == "train")
        ref = Q.run(ref_mod, name, stage)
        mine = Q.reference(name, stage, mode, torch.float32)
        what = "%s %s %s" % (name, stage, mode)
        assert all(torch.equal(a, b) for a, b in zip(ref["outs"], mine["outs"])) and torch.equal(ref["loss"], mine["loss"]), what
        assert list(ref["inputs"]) == list(Q.INPUTS[stage]) == list(mine["inputs"])
        for k, g in ref["inputs"].items():
            assert g is not None and torch.equal(g, mine["inputs"][k]), "restatement's gradient of %s differs from the reference: %s" % (k, what)
        assert list(ref["grads"]) == list(mine["grads"])
        for k, g in ref["grads"].items():
            assert torch.equal(g, mine["grads"][k]), "restatement's gradient of %s differs from the reference: %s" % (k, what)
        for k, v in ref["buffers"].items():
            assert torch.equal(v, mine["buffers"][k]), (what, k)
        f64 = Q.reference(name, stage, mode, torch.float64)
        n, tight = Q.whole_network_rule(Q.yardstick_tensors(mine, mode), Q.yardstick_tensors(f64, mode), Q.yardstick_tensors(mine, mode),
                                         what + ": FP32 restatement")
        worst = max((g.double() - f64["grads"][k]).abs().max().item() / max(f64["grads"][k].abs().max().item(), 1e-30)
                    for k, g in ref["grads"].items() if not Q.zero_by_construction(k, mode))
        print("%s: restatement == reference (%d inputs, %d parameters); loss %.6g; FP32 vs FP64 gradients: worst %.3g of a tensor's range"
              % (what, len(ref["inputs"]), len(ref["grads"]), ref["loss"].item(), worst))
        prefix = "%s/%s/%s/" % (name, stage, mode)
        out[prefix + "loss"] = ref["loss"].numpy()
        for k, g in ref["inputs"].items():
            out[prefix + "in/" + k] = g.numpy()
        out[prefix + "p/names"], out[prefix + "p/stats"], out[prefix + "p/samples"] = Q.packed(prefix, ref["grads"])
        if mode == "train":
            used = sorted({k.rsplit(".", 2)[0] for k in ref["grads"]})     # the modules the stage runs
            keys = [k for k in ref["buffers"] if any(k.startswith(u + ".") for u in used)]
            out[prefix + "b/names"] = np.array(keys)
            for i, k in enumerate(keys):
                out[prefix + "b/%d" % i] = ref["buffers"][k].numpy()
    path = os.path.join(ROOT, "tests", "golden", "deeppruner_processor_bwd.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
