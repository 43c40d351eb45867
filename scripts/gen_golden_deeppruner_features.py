"""Record tests/golden/deeppruner_features.npz from the REAL reference ``DeepPrunerBestBackbone``, ``DeepPrunerFastBackbone``
(dmb/modeling/stereo/backbones/DeepPruner.py) and ``DeepPrunerRefinement`` (dmb/modeling/stereo/disp_refinement/DeepPruner.py), on
the CPU at 8 threads.

Recorded: the ``state_dict`` names and shapes of the three classes; per refinement case of tests/_deeppruner_features_ref.py
(``REFINE_CASES``) every up-sampled map the cascade appends and, taken with a forward hook, every refined map before its
up-sampling (what the ReLU clamps); per backbone case (``BACKBONE_CASES``) strided sub-samples of the feature and of every
low-level map, with their full shapes.  Inputs and weights are regenerated from their seeds, not stored.  The script asserts that
the restatement equals the reference bit for bit and that every refined map holds clamped zeros and positive values, and prints
the reference's distance from the FP64 yardstick.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_deeppruner_features.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import _deeppruner_features_ref as R  # noqa: E402


def _keys(module):
    sd = module.state_dict()
    return np.array(list(sd)), np.array([",".join(str(s) for s in t.shape) for t in sd.values()])


def _report(key, rec, f64):
    d = (rec.double() - f64).abs()
    print("  %-22s %-18s max|fp64| %.4g  reference vs FP64: max %.3g mean %.3g  non-zero %.1f %%"
          % (key, tuple(rec.shape), f64.abs().max(), d.max(), d.mean(), 100 * (rec != 0).float().mean()))


def main():
    import_reference()
    from dmb.modeling.stereo.backbones import DeepPruner as ref_backbones
    from dmb.modeling.stereo.disp_refinement.DeepPruner import DeepPrunerRefinement

    torch.set_num_threads(8)
    out = {}
    for name, ((planes, num, B, (H, W)), _) in R.REFINE_CASES.items():
        ref = R.seeded_state(DeepPrunerRefinement(list(planes), True, num), R.WEIGHT_SEED).eval()
        mine = R.refinement(name)
        if num == 2:
            out["refinement/keys"], out["refinement/shapes"] = _keys(ref)
        assert list(ref.state_dict()) == list(mine.state_dict())
        refined = []
        hooks = [blk.register_forward_hook(lambda m, i, o: refined.append(o)) for blk in ref.refine_blocks]
        disps, fms = R.refine_inputs(name)
        kept = [t.clone() for t in fms]
        with torch.no_grad():
            got = ref(list(disps), fms)
            want = mine(list(disps), fms)
            stages = mine.stages(disps, fms)
        for h in hooks:
            h.remove()
        assert len(got) == num + 1 and got[-1] is disps[0] and all(torch.equal(a, b) for a, b in zip(kept, fms))
        f64 = R.fp64_refinement(name)
        print("%s: %s, num %d" % (name, planes, num))
        for i in range(num):
            up = got[num - 1 - i]                                   # reversed: the last stage first
            assert up.shape == (B, 1, (H << i) * 2, (W << i) * 2) and refined[i].shape == (B, 1, H << i, W << i)
            assert torch.equal(up, want[num - 1 - i]) and torch.equal(refined[i], stages[i][0]) and torch.equal(up, stages[i][1]), \
                "restatement differs from the reference: %s stage %d" % (name, i)
            clamped = (refined[i] == 0).float().mean().item()
            assert 0.05 <= clamped <= 0.95, (name, i, clamped)      # both clamped zeros and positive values
            out["%s/refined%d" % (name, i)], out["%s/up%d" % (name, i)] = refined[i].numpy(), up.numpy()
            _report("refined%d" % i, refined[i], f64[i][0])
            _report("up%d" % i, up, f64[i][1])
    for name, (cls, shape, _, strides) in R.BACKBONE_CASES.items():
        ref = R.seeded_state(getattr(ref_backbones, cls)(3, True), R.WEIGHT_SEED).eval()
        mine = R.backbone(name)
        out[name + "/keys"], out[name + "/shapes"] = _keys(ref)
        assert list(ref.state_dict()) == list(mine.state_dict())
        x = R.backbone_input(name)
        with torch.no_grad():
            (got, _), (want, _) = (R.flatten(o) for o in ref(x, x)), (R.flatten(o) for o in mine(x, x))
        assert len(got) == len(want) == len(strides)
        f64 = R.fp64_backbone(name)
        print("%s: %s at %s" % (name, cls, shape))
        out[name + "/full_shapes"] = np.array([list(t.shape) for t in got])
        for i, (a, b, sub) in enumerate(zip(got, want, R.subsample(name, got))):
            assert torch.equal(a, b), "restatement differs from the reference: %s map %d" % (name, i)
            out["%s/map%d" % (name, i)] = sub.contiguous().numpy()
            _report("map%d (sub-sampled)" % i, sub, f64[i])
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN))


if __name__ == "__main__":
    main()
