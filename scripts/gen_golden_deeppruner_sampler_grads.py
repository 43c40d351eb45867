"""Record tests/golden/deeppruner_sampler_grads.npz from the REAL reference DeepPrunerSampler (dmb/modeling/stereo/disp_samplers)
under autograd, on the CPU at 8 threads.

As in gen_golden_deeppruner_sampler.py the one draw of PatchMatch's noise is replaced by a seeded tensor; the rest of the module
runs as it is.  Recorded, for the small cases of tests/_deeppruner_sampler_bwd_cases.py: stage "pre" -- the output, the upstream
gradient and the gradients of ``left`` and ``right`` (the reference draws its noise inside, so it has no gradient for it); stage
"post" -- the output, the upstream gradient and the gradients of the two range maps.  Inputs are regenerated from their seeds.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_deeppruner_sampler_grads.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import _deeppruner_ref as R  # noqa: E402
from tests import _deeppruner_sampler_bwd_cases as K  # noqa: E402


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
    for name, (shape, P, max_disp) in K.CHAIN_CASES.items():
        seed = K.chain_seed(name)
        left, right, noise, g = K.chain_inputs(name, seed)
        draw["noise"] = noise
        sampler = DeepPrunerSampler(max_disp=max_disp, batch_norm=True, propagation_filter_size=3, iterations=R.ITERATIONS,
                                    temperature=R.TEMPERATURE, patch_match_disparity_sample_number=P + 2,
                                    uniform_disparity_sample_number=R.UNIFORM_SAMPLES).eval()
        left, right = left.requires_grad_(), right.requires_grad_()
        pre = sampler('pre', left, right)
        dl, dr = torch.autograd.grad(pre, (left, right), g)
        out.update({name + "/seed": np.array(seed), name + "/pre": pre.detach().numpy(), name + "/g": g.numpy(),
                    name + "/d_left": dl.numpy(), name + "/d_right": dr.numpy()})
        mine = K.chain_grads(name, seed, torch.float32)
        print(name, "seed", seed, "restatement vs reference: out %.3g d_left %.3g d_right %.3g" % (
            (mine[0] - pre.detach()).abs().max(), (mine[1] - dl).abs().max(), (mine[2] - dr).abs().max()))
    for name, (shape, N, max_disp, seed) in K.POST_CASES.items():
        lo, hi, g = K.post_inputs(name)
        sampler = DeepPrunerSampler(max_disp=max_disp, uniform_disparity_sample_number=N).eval()
        lo, hi = lo.requires_grad_(), hi.requires_grad_()
        dummy = torch.zeros((shape[0], 4) + shape[2:])
        post = sampler('post', dummy, dummy, lo, hi)
        dlo, dhi = torch.autograd.grad(post, (lo, hi), g)
        out.update({name + "/post": post.detach().numpy(), name + "/g": g.numpy(), name + "/d_lo": dlo.numpy(),
                    name + "/d_hi": dhi.numpy()})
        mine = K.post_grads(lo.detach(), hi.detach(), g, N, max_disp, torch.float32)
        print(name, "restatement vs reference: out %.3g d_lo %.3g d_hi %.3g" % (
            (mine[0] - post.detach()).abs().max(), (mine[1] - dlo).abs().max(), (mine[2] - dhi).abs().max()))
    path = os.path.join(ROOT, 'tests', 'golden', 'deeppruner_sampler_grads.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
