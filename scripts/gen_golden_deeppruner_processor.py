"""Record tests/golden/deeppruner_processor.npz from the REAL reference ``DeepPrunerProcessor`` and ``ConfidenceRangePredictor``
(dmb/modeling/stereo/cost_processors/DeepPruner.py), on the CPU at 8 threads.

Recorded: the ``state_dict`` names and shapes of both classes, and per case of tests/_deeppruner_processor_ref.py (``CASES``) the six
FP32 outputs (stage "pre": min_disparity, max_disparity and the two feature maps; stage "post", fed those two feature maps:
disparity and its feature map) and the three costs that feed the soft arg-mins (taken with forward hooks).  Inputs and weights are
regenerated from their seeds (``case_inputs``, ``seeded_state``), not stored.  The script asserts that the restatement equals the
reference bit for bit, checks the conditions the CPU test puts on the inputs, and prints the reference's distance from the FP64
yardstick.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_deeppruner_processor.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import attrdict, import_reference  # noqa: E402
from tests import _deeppruner_processor_ref as R  # noqa: E402


def _keys(module):
    sd = module.state_dict()
    return np.array(list(sd)), np.array([",".join(str(s) for s in t.shape) for t in sd.values()])


def _cfg(C, P, N):
    hp = R.HOURGLASS_IN_PLANES
    return attrdict(dict(model=dict(batch_norm=True, cost_processor=dict(
        type="DeepPruner", patch_match_disparity_sample_number=P, uniform_disparity_sample_number=N,
        confidence_range_predictor=dict(in_planes=2 * C + 1, hourglass_in_planes=hp),
        cost_aggregator=dict(type="DeepPruner", in_planes=2 * C + 2 * P + 1, hourglass_in_planes=hp)))))


def main():
    import_reference()
    from dmb.modeling.stereo.cost_processors.DeepPruner import ConfidenceRangePredictor, DeepPrunerProcessor

    torch.set_num_threads(8)
    out = {}
    for name, ((B, C, P, N, H, W), _) in R.CASES.items():
        ref = R.seeded_state(DeepPrunerProcessor(_cfg(C, P, N)), R.WEIGHT_SEED).eval()
        mine = R.processor(name)
        if "processor/keys" not in out:
            out["processor/keys"], out["processor/shapes"] = _keys(ref)
            out["predictor/keys"], out["predictor/shapes"] = _keys(ConfidenceRangePredictor(2 * C + 1, R.HOURGLASS_IN_PLANES, P))
            assert len(out["processor/keys"]) == 258
        assert list(_keys(ref)[0]) == list(out["processor/keys"]) == list(mine.state_dict())     # the same 258 names at any counts
        seen = {}
        crp = ref.confidence_range_predictor
        hooks = [crp.min_disparity_predictor.register_forward_hook(lambda m, i, o: seen.__setitem__("pre/cost_for_min", o.squeeze(1))),
                 crp.max_disparity_predictor.register_forward_hook(lambda m, i, o: seen.__setitem__("pre/cost_for_max", o.squeeze(1))),
                 ref.cost_aggregator.register_forward_hook(lambda m, i, o: seen.__setitem__("post/cost", o[0]))]
        left, right, pre, post = R.case_inputs(name)
        with torch.no_grad():
            got = list(ref("pre", left, right, pre))
            got += list(ref("post", left, right, post, got[2], got[3]))
            want = list(mine("pre", left, right, pre))
            want += list(mine("post", left, right, post, want[2], want[3]))
            mask = (R.raw_volume(left, right, pre)[:, C:2 * C] > 0).float().mean().item()
        for h in hooks:
            h.remove()
        assert got[0].shape == (B, 1, H, W) and got[2].shape == (B, P, H, W)
        assert got[4].shape == (B, 1, 2 * H, 2 * W) and got[5].shape == (B, N, 2 * H, 2 * W)
        for key, a, b in zip(R.OUTPUTS, got, want):
            assert torch.equal(a, b), "restatement differs from the reference: %s %s" % (name, key)
            out["%s/%s" % (name, key)] = a.numpy()
        for key in R.COSTS:
            out["%s/%s" % (name, key)] = seen[key].numpy()
        np.savez_compressed(R.GOLDEN, **out)       # (fp64_outputs reads the pre-stage features of this case from the file)
        f64 = R.fp64_outputs(name)
        print("%s: the warp keeps %.1f %% of the left channels" % (name, 100 * mask))
        for key in R.COSTS + R.OUTPUTS:
            t = torch.from_numpy(out["%s/%s" % (name, key)])
            d = (t.double() - f64[key]).abs()
            print("  %-18s %-18s max|fp64| %.4g  reference vs FP64: max %.3g mean %.3g  non-zero %.1f %%"
                  % (key, tuple(t.shape), f64[key].abs().max(), d.max(), d.mean(), 100 * (t != 0).float().mean()))
            share = (t != 0).float().mean().item()
            assert share == 1.0 if "disparity" in key else (share >= 0.3 or key in R.COSTS), (name, key, share)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN))


if __name__ == "__main__":
    main()
