"""Record tests/golden/deeppruner_loss.npz from the REAL reference: the training tail of dmb/modeling/stereo/models/DeepPruner.py
(:82-108) -- its own F.interpolate sequence, its DispSmoothL1Loss (built by make_gsm_loss_evaluator's factory with the case's
weights) and its quantile_loss -- on the CPU with autograd, for the recorded cases of tests/_deeppruner_loss_ref.py.

Per case: the reference's FP32 loss dict (quantile_loss, l1_loss_lvl0 ..) and the FP32 gradients of ``R.total`` of it with respect
to the K list maps and the two range maps; the same from the restatement in FP64 (the yardstick).  Per case also an "empty" run, a
ground truth with no valid pixel: the reference's losses (0 per smooth-L1 level, NaN for the quantile loss) and the largest
gradient magnitude (0).  Inputs are regenerated from their seeds, not stored.  The script asserts that
  - the FP32 restatement equals the reference bit for bit, losses and gradients,
  - every branch (|v - gt| < 1 per level, gt - M < 0 per range map) holds between 10 % and 90 % of the valid pixels, and both masks
    exclude something on each side,
and prints the reference's distance from the FP64 yardstick.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_deeppruner_loss.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import _deeppruner_loss_ref as R  # noqa: E402


def reference_run(name, ref_l1, ref_quantile, empty=False):
    """models/DeepPruner.py:82-108 as it stands, on the case's seeded maps."""
    disps, min_disparity, max_disparity, target = R.inputs(name, torch.float32, empty)
    leaves = [t.requires_grad_() for t in disps + [min_disparity, max_disparity]]
    _, _, _, _, weights, theta, _ = R.CASES[name]
    H, W = target.shape[-2:]
    disps = list(disps)
    min_disparity = F.interpolate(min_disparity * W / min_disparity.shape[-1], size=(H, W), mode='bilinear', align_corners=False)
    max_disparity = F.interpolate(max_disparity * W / max_disparity.shape[-1], size=(H, W), mode='bilinear', align_corners=False)
    disps.extend([min_disparity, max_disparity])
    disps = [F.interpolate(d * W / d.shape[-1], size=(H, W), mode='bilinear', align_corners=False) for d in disps]
    loss_dict = dict(quantile_loss=ref_quantile(min_disparity, max_disparity, target, max_disp=R.MAX_DISP, theta=theta, weight=1.0))
    evaluator = ref_l1(max_disp=R.MAX_DISP, weights=weights, sparse=False)
    loss_dict.update({k: v * 1.0 for k, v in evaluator(disps, target).items()})     # CombinedLossEvaluators, weight 1.0
    R.total(loss_dict).backward()
    return [v.detach() for v in loss_dict.values()], [t.grad for t in leaves], list(loss_dict)


def main():
    import_reference()
    from dmb.modeling.stereo.losses.smooth_l1_loss import DispSmoothL1Loss
    from dmb.modeling.stereo.losses.utils.quantile_loss import quantile_loss

    torch.set_num_threads(8)
    out = {}
    for name in R.RECORDED:
        K = len(R.CASES[name][1])
        fractions, excluded, low, high = R.branch_fractions(name)
        assert all(0.1 <= f <= 0.9 for f in fractions), (name, fractions)
        assert low > 0 and high > 0, (name, low, high)
        ref_loss, ref_grad, keys = reference_run(name, DispSmoothL1Loss, quantile_loss)
        assert keys == ["quantile_loss"] + ["l1_loss_lvl%d" % i for i in range(K + 2)]
        my_loss, my_grad = R.run(name, torch.float32)
        assert all(torch.equal(a, b) for a, b in zip(ref_loss, my_loss)), "restatement differs from the reference: %s losses" % name
        assert all(torch.equal(a, b) for a, b in zip(ref_grad, my_grad)), "restatement differs from the reference: %s gradients" % name
        loss64, grad64 = R.run(name, torch.float64)
        out[name + "/keys"] = np.array(keys)
        out[name + "/loss32"] = torch.stack(ref_loss).numpy()
        out[name + "/loss64"] = torch.stack(loss64).numpy()
        for i, (g32, g64) in enumerate(zip(ref_grad, grad64)):
            out["%s/grad32_%d" % (name, i)], out["%s/grad64_%d" % (name, i)] = g32.numpy(), g64.numpy()
        out[name + "/fractions"] = np.array(fractions + [excluded, low, high])
        e_loss, e_grad, _ = reference_run(name, DispSmoothL1Loss, quantile_loss, empty=True)
        m_loss, m_grad = R.run(name, torch.float32, empty=True)
        assert all(torch.equal(a, b) or (torch.isnan(a) and torch.isnan(b)) for a, b in zip(e_loss, m_loss)), name
        assert all(torch.equal(a, b) for a, b in zip(e_grad, m_grad)), name
        out[name + "/empty_loss32"] = torch.stack(e_loss).numpy()
        out[name + "/empty_grad_max"] = np.array([g.abs().max().item() for g in e_grad])
        print("%s: %d + 2 maps, %.1f %% of the pixels excluded (%.1f %% <= 0, %.1f %% >= %d); branch shares %s"
              % (name, K, 100 * excluded, 100 * low, 100 * high, R.MAX_DISP, " ".join("%.2f" % f for f in fractions)))
        for k, a, b in zip(keys, ref_loss, loss64):
            print("  %-14s fp64 %.9g  reference vs FP64 %.3g" % (k, b.item(), abs(a.double().item() - b.item())))
        for i, (g32, g64) in enumerate(zip(ref_grad, grad64)):
            print("  grad %d %-16s max|fp64| %.4g  reference vs FP64: max %.3g" % (i, tuple(g64.shape), g64.abs().max(),
                                                                                  (g32.double() - g64).abs().max()))
        print("  empty mask: losses %s, largest gradient %g" % (out[name + "/empty_loss32"], out[name + "/empty_grad_max"].max()))
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN))


if __name__ == "__main__":
    main()
