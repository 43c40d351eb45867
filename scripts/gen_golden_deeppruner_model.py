"""Record tests/golden/deeppruner_model.npz from the REAL reference ``DeepPruner`` model (dmb/modeling/stereo/models/DeepPruner.py)
built from the reference's own two config files, on the CPU at 8 threads, in eval mode.

The reference draws PatchMatch's noise inside DisparityInitialization.forward; that one draw is replaced by a seeded tensor (as
scripts/gen_golden_deeppruner_sampler.py does), the rest of the model runs as it is.  Recorded per case of
tests/_deeppruner_model_ref.py (``CASES``): the ``state_dict`` names and shapes, the full shape of every output map, every output
map sub-sampled with the case's odd strides, the two feature-size range maps whole, and the reference's ``target > 0`` decisions
at the voxels of the two raw volumes whose warped value is nearly zero (what the FP64 yardstick takes from the reference, see
tests/_deeppruner_model_ref.py).  Images, noise and weights are regenerated from their seeds, not stored.  The script asserts that
  - the restatement equals the reference bit for bit in FP32 (every full map, both range maps),
  - the inputs are not degenerate: min < max on most pixels, every refined map holds clamped zeros and positive values, the two
    residual maps are not all zero,
  - (Mn * W) / W differs from Mn on at least one recorded pixel (the second scaling of the range maps is observable),
and prints the reference's distance from the FP64 yardstick.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_deeppruner_model.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference, load_cfg  # noqa: E402
from tests import _deeppruner_model_ref as R  # noqa: E402


def main():
    import_reference()
    from dmb.modeling.stereo.disp_samplers.utils import patch_match as ref_pm
    from dmb.modeling.stereo.models.DeepPruner import DeepPruner

    draw = {}
    init_forward = ref_pm.DisparityInitialization.forward

    def seeded_forward(self, min_disparity, max_disparity):
        _, interval_min, interval = init_forward(self, min_disparity, max_disparity)
        return draw["noise"].clone(), interval_min, interval

    ref_pm.DisparityInitialization.forward = seeded_forward
    torch.set_num_threads(8)
    out = {}
    for name, (rel, _, _, planes, shape, seed, strides) in R.CASES.items():
        ref = R.seeded_model(DeepPruner(load_cfg(rel))).eval()
        mine = R.model(name)
        sd = ref.state_dict()
        assert list(sd) == list(mine.state_dict()) and all(torch.equal(a, b) for a, b in zip(sd.values(), mine.state_dict().values()))
        out[name + "/keys"] = np.array(list(sd))
        out[name + "/shapes"] = np.array([",".join(str(s) for s in t.shape) for t in sd.values()])
        left, right, noise = R.inputs(name)
        draw["noise"] = noise
        seen = {}
        hook = ref.cost_processor.confidence_range_predictor.register_forward_hook(
            lambda m, i, o: seen.update(min_disparity=o[0], max_disparity=o[1]))
        with torch.no_grad():
            got, _ = ref(dict(leftImage=left, rightImage=right))
        hook.remove()
        want = R.fp32_outputs(name)
        K, (B, _, H, W) = len(planes) + 1, shape
        assert got["costs"] == [None] and len(got["disps"]) == len(want["disps"]) == K + 4
        for i, (a, b) in enumerate(zip(got["disps"], want["disps"])):
            assert a.shape == (B, 1, H, W) and torch.equal(a, b), "restatement differs from the reference: %s map %d" % (name, i)
        for key in ("min_disparity", "max_disparity"):
            assert torch.equal(seen[key], want[key]), "restatement differs from the reference: %s %s" % (name, key)
            out["%s/%s" % (name, key)] = seen[key].numpy()
        lo, hi = seen["min_disparity"], seen["max_disparity"]
        ordered = (lo < hi).float().mean().item()
        assert ordered >= 0.6, (name, ordered)
        for i in range(K - 1):                                            # the refined maps: clamped zeros and positive values
            zeros = (got["disps"][i] == 0).float().mean().item()
            assert 0.005 <= zeros <= 0.995, (name, i, zeros)
        assert all(got["disps"][i].abs().max() > 0 for i in (K + 2, K + 3))
        Mn, Mx = R.up(lo, (H, W)), R.up(hi, (H, W))
        moved = sum(int((a != b).sum()) for a, b in zip(R.subsample(name, got["disps"][K:K + 2]), R.subsample(name, [Mn, Mx])))
        assert moved >= 1, name
        out[name + "/full_shapes"] = np.array([list(t.shape) for t in got["disps"]])
        for i, sub in enumerate(R.subsample(name, got["disps"])):
            out["%s/disp%d" % (name, i)] = sub.contiguous().numpy()
        # the FP64 run with the reference's whole masks; then the voxels where it could have decided otherwise
        with torch.no_grad():
            whole = R.model(name, torch.float64)(*R.inputs(name, torch.float64), masks=want["masks"])
        for v, t64, m32 in zip(("pre", "post"), whole["targets"], want["masks"]):
            near, differs = (t64 != 0) & (t64.abs() < R.NEAR_ZERO), (t64 > 0) != m32
            index = torch.nonzero((near | differs).reshape(-1)).squeeze(1)
            out["%s/%s_index" % (name, v)], out["%s/%s_decision" % (name, v)] = index.numpy(), m32.reshape(-1)[index].numpy()
            print("%s %s volume: %d of %d voxels nearly zero, the FP64 sign differs from the reference's at %d (%d of them not nearly zero)"
                  % (name, v, int(near.sum()), t64.numel(), int(differs.sum()), int((differs & ~near).sum())))
        np.savez_compressed(R.GOLDEN, **out)       # (fp64_outputs reads this case's decisions from the file)
        f64 = R.fp64_outputs(name)
        assert all(torch.equal(a, b) for a, b in zip(f64["disps"], whole["disps"])), "the recorded decisions do not reproduce the masks"
        print("%s: %s at %s, %d keys; min < max on %.1f %%; (M * W) / W != M on %d recorded pixels"
              % (name, rel, shape, len(sd), 100 * ordered, moved))
        for i, (sub, sub64) in enumerate(zip(R.subsample(name, got["disps"]), R.subsample(name, f64["disps"]))):
            d, full = (sub.double() - sub64).abs(), (got["disps"][i].double() - f64["disps"][i]).abs()
            print("  disp%d %-16s max|fp64| %.4g  reference vs FP64 (sub-sampled): max %.3g mean %.3g  (whole: max %.3g)  zeros %.1f %%"
                  % (i, tuple(sub.shape), sub64.abs().max(), d.max(), d.mean(), full.max(), 100 * (sub == 0).float().mean()))
        for key in ("min_disparity", "max_disparity"):
            d = (seen[key].double() - f64[key]).abs()
            print("  %-21s max|fp64| %.4g  reference vs FP64: max %.3g mean %.3g" % (key, f64[key].abs().max(), d.max(), d.mean()))
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN))


if __name__ == "__main__":
    main()
