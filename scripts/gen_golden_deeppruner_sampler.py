"""Record tests/golden/deeppruner_sampler.npz from the REAL reference DeepPrunerSampler (dmb/modeling/stereo/disp_samplers), on
the CPU at 8 threads.

The reference draws PatchMatch's noise inside DisparityInitialization.forward; that one draw is replaced by a seeded tensor, the
rest of the module runs as it is.  Recorded: the FP32 outputs of stage "pre" and stage "post" for the cases of
tests/_deeppruner_ref.py (``GOLDEN_CASES``).  Inputs are regenerated from their seeds (``golden_inputs``), not stored.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_deeppruner_sampler.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import _deeppruner_ref as R  # noqa: E402


def main():
    import_reference()
    from dmb.modeling.stereo.disp_samplers.DeepPruner import DeepPrunerSampler
    from dmb.modeling.stereo.disp_samplers.utils import patch_match as ref_pm

    draw = {}
    init_forward = ref_pm.DisparityInitialization.forward

    def seeded_forward(self, min_disparity, max_disparity):
        _, interval_min, interval = init_forward(self, min_disparity, max_disparity)
        return draw["noise"].clone(), interval_min, interval

    ref_pm.DisparityInitialization.forward = seeded_forward
    torch.set_num_threads(8)
    out = {}
    for name, (shape, max_disp, scale, seed) in R.GOLDEN_CASES.items():
        left, right, noise, lo, hi = R.golden_inputs(name)
        draw["noise"] = noise
        sampler = DeepPrunerSampler(max_disp=max_disp, batch_norm=True, propagation_filter_size=3, iterations=R.ITERATIONS,
                                    temperature=R.TEMPERATURE, patch_match_disparity_sample_number=R.PATCH_MATCH_SAMPLES,
                                    uniform_disparity_sample_number=R.UNIFORM_SAMPLES).eval()
        with torch.no_grad():
            pre = sampler('pre', left, right)
            post = sampler('post', left, right, lo, hi)
        assert pre.shape == (shape[0], R.PATCH_MATCH_SAMPLES) + shape[2:] and post.shape == (shape[0], R.UNIFORM_SAMPLES) + shape[2:]
        out[name + "/pre"], out[name + "/post"] = pre.numpy(), post.numpy()
        out[name + "/seed"] = np.array(seed)
        with torch.no_grad():
            mine = R.sampler('pre', left, right, noise=noise, max_disp=max_disp)
            f64 = R.sampler('pre', *(t.double() for t in (left, right)), noise=noise.double(), max_disp=max_disp)
        print(name, "restatement == reference:", torch.equal(mine, pre),
              torch.equal(R.sampler('post', left, right, lo, hi, max_disp=max_disp), post),
              " reference vs FP64: max %.3g mean %.3g" % ((pre - f64).abs().max(), (pre - f64).abs().mean()))
    path = os.path.join(ROOT, 'tests', 'golden', 'deeppruner_sampler.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
