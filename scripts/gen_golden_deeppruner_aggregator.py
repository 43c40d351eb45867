"""Record tests/golden/deeppruner_aggregator.npz from the REAL reference DeepPrunerAggregator and HWHourglass
(dmb/modeling/stereo/cost_processors), on the CPU at 8 threads.

Recorded: the FP32 outputs for the cases of tests/_hw_ref.py (``GOLDEN_CASES``, ``HOURGLASS_CASES``) and the ``state_dict`` names
and shapes of both modules.  Inputs and weights are regenerated from their seeds (``golden_input``, ``seeded_state``), not stored.
The script asserts that the restatement of tests/_hw_ref.py equals the reference bit for bit, and prints the reference's distance
from an FP64 evaluation of the same weights.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_deeppruner_aggregator.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import _hw_ref as R  # noqa: E402


def _keys(module):
    sd = module.state_dict()
    return np.array(list(sd)), np.array([",".join(str(s) for s in t.shape) for t in sd.values()])


def main():
    import_reference()
    from dmb.modeling.stereo.cost_processors.aggregators.DeepPruner import DeepPrunerAggregator
    from dmb.modeling.stereo.cost_processors.utils.hw_hourglass import HWHourglass

    torch.set_num_threads(8)
    agg = R.seeded_state(DeepPrunerAggregator(R.IN_PLANES, R.HOURGLASS_IN_PLANES, batch_norm=True), R.WEIGHT_SEED).eval()
    hg = R.seeded_state(HWHourglass(R.HOURGLASS_IN_PLANES, batch_norm=True), R.WEIGHT_SEED + 1).eval()
    out = {}
    out["aggregator/keys"], out["aggregator/shapes"] = _keys(agg)
    out["hourglass/keys"], out["hourglass/shapes"] = _keys(hg)
    assert list(out["aggregator/keys"]) == list(R.aggregator().state_dict()) and len(out["aggregator/keys"]) == 85
    assert list(out["hourglass/keys"]) == list(R.hourglass().state_dict())
    for name in list(R.GOLDEN_CASES) + list(R.HOURGLASS_CASES):
        x = R.golden_input(name)
        with torch.no_grad():
            if name in R.GOLDEN_CASES:
                (ref,), (mine,) = agg(x), R.aggregator()(x)
                assert ref.shape == (x.shape[0],) + tuple(x.shape[2:])
            else:
                ref, mine = hg(x), R.hourglass()(x)
                assert ref.shape == x.shape
        assert torch.equal(ref, mine), "restatement differs from the reference: %s" % name
        f64 = R.fp64_output(name)
        d = (ref.double() - f64).abs()
        print("%s %s: restatement == reference; max|out| %.4g; reference vs FP64: max %.3g mean %.3g"
              % (name, tuple(x.shape), f64.abs().max(), d.max(), d.mean()))
        out[name + "/out"] = ref.numpy()
    path = os.path.join(ROOT, "tests", "golden", "deeppruner_aggregator.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
