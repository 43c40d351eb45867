"""Record tests/golden/deeppruner_refinement_bwd.npz from the REAL reference ``DeepPrunerRefinement``
(dmb/modeling/stereo/disp_refinement/DeepPruner.py): forward + backward on the CPU at 8 threads, in train() and eval(), on the runs
of tests/_deeppruner_refinement_bwd_ref.py (``RUNS``; its docstring lists the keys).  The loss is a fixed seeded projection of every
returned map.

Data only: the loss, the incoming disparity's gradient in full, per feature map and per parameter the gradient's sum, its largest
magnitude and entries at seeded positions, the updated running buffers.  Inputs, weights and the projections are regenerated from
their seeds, never stored.

The script asserts that autograd through the restatement of tests/_deeppruner_features_ref.py equals the reference's maps, loss,
gradients and buffers bit for bit: that makes the restatement the yardstick everywhere else.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_deeppruner_refinement_bwd.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import _deeppruner_features_ref as R  # noqa: E402
from tests import _deeppruner_refinement_bwd_ref as Q  # noqa: E402
from tests._hw_bwd_ref import whole_network_rule  # noqa: E402


def main():
    import_reference()
    from dmb.modeling.stereo.disp_refinement.DeepPruner import DeepPrunerRefinement

    torch.set_num_threads(8)
    out = {}
    for name, mode in Q.RUNS:
        (planes, num, _, _), _ = R.REFINE_CASES[name]
        ref_mod = Q.fill(DeepPrunerRefinement(list(planes), True, num)).train(mode == "train")
        ref = Q.run(ref_mod, name)
        mine = Q.reference(name, mode, torch.float32)
        what = "%s %s" % (name, mode)
        assert len(ref["outs"]) == num + 1 == len(mine["outs"])
        assert all(torch.equal(a, b) for a, b in zip(ref["outs"], mine["outs"])) and torch.equal(ref["loss"], mine["loss"]), what
        assert list(ref["inputs"]) == list(Q.inputs_of(name)) == list(mine["inputs"])
        for k, g in ref["inputs"].items():
            assert g is not None and torch.equal(g, mine["inputs"][k]), "restatement's gradient of %s differs from the reference: %s" % (k, what)
        assert list(ref["grads"]) == list(mine["grads"]) == [k for k, _ in ref_mod.named_parameters()]
        for k, g in ref["grads"].items():
            assert torch.equal(g, mine["grads"][k]), "restatement's gradient of %s differs from the reference: %s" % (k, what)
        for k, v in ref["buffers"].items():
            assert torch.equal(v, mine["buffers"][k]), (what, k)
        f64 = Q.reference(name, mode, torch.float64)
        n, tight = whole_network_rule(Q.tensors(mine), Q.tensors(f64), Q.tensors(mine), what + ": FP32 restatement")
        worst = max((g.double() - Q.tensors(f64)[k]).abs().max().item() / max(Q.tensors(f64)[k].abs().max().item(), 1e-30)
                    for k, g in Q.tensors(ref).items())
        print("%s: restatement == reference (%d inputs, %d parameters); loss %.6g; FP32 vs FP64 gradients: worst %.3g of a tensor's range"
              % (what, len(ref["inputs"]), len(ref["grads"]), ref["loss"].item(), worst))
        prefix = "%s/%s/" % (name, mode)
        out[prefix + "loss"] = ref["loss"].numpy()
        out[prefix + "in/disp"] = ref["inputs"]["disp"].numpy()
        fms = {k: g for k, g in ref["inputs"].items() if k != "disp"}
        out[prefix + "in/names"], out[prefix + "in/stats"], out[prefix + "in/samples"] = Q.packed(prefix, fms, Q.IN_SAMPLES)
        out[prefix + "p/names"], out[prefix + "p/stats"], out[prefix + "p/samples"] = Q.packed(prefix, ref["grads"])
        if mode == "train":
            keys = list(ref["buffers"])
            out[prefix + "b/names"] = np.array(keys)
            for i, k in enumerate(keys):
                out[prefix + "b/%d" % i] = ref["buffers"][k].numpy()
    path = os.path.join(ROOT, "tests", "golden", "deeppruner_refinement_bwd.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
