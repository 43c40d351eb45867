"""Record tests/golden/anynet.npz from the REAL reference AnyNet (configs/AnyNet/scene_flow.py of the reference tree), on the CPU.

Seeded weights, BatchNorm statistics with gammas of both signs and betas large enough that relu(beta) != 0 at the borders.  The
reference's SPN op is CUDA-only, so the oracle's restatement (oracle/dmb_oracle.py: spn_gaterecurrent2d) stands in for it.
Records the state_dict (names, shapes, dtypes, values), the stage-boundary tensors of one FP32 forward at batch 2 x 64x128 and the
same forward in FP64.  Inputs are regenerated from seeds (tests/_anynet_ref.py: ``golden_inputs``).

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_anynet.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import dmb_oracle as O  # noqa: E402
from oracle.gen_golden import import_reference, load_cfg  # noqa: E402
from tests._anynet_ref import golden_inputs  # noqa: E402

SHAPE = (2, 3, 64, 128)
SEED = 1234


def seeded_state(model, seed=SEED):
    """Conv weights ~ N(0, 1/fan_in) (x1.5), biases ~ N(0, 0.1); BatchNorm gamma U(-1.5, 1.5), beta N(0.3, 0.5), mean N(0, 0.3),
    var U(0.5, 2)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        if k.endswith('num_batches_tracked') or 'disp_regression' in k:
            sd[k] = v.clone()
        elif k.endswith('running_mean'):
            sd[k] = torch.randn(v.shape, generator=g) * 0.3
        elif k.endswith('running_var'):
            sd[k] = torch.rand(v.shape, generator=g) * 1.5 + 0.5
        elif v.dim() == 1 and k.endswith('.weight'):      # BatchNorm gamma
            sd[k] = torch.rand(v.shape, generator=g) * 3.0 - 1.5
        elif v.dim() == 1:
            sd[k] = torch.randn(v.shape, generator=g) * (0.5 if 'agg' not in k else 0.1) + (0.3 if 'agg' not in k else 0.0)
        else:
            fan_in = v[0].numel()
            sd[k] = torch.randn(v.shape, generator=g) * (1.5 / fan_in ** 0.5)
            if 'classify' in k:       # a residual small next to the disparity: relu(res + init) is not 0 everywhere
                sd[k] = sd[k] * 0.02
    return sd


def inputs(dtype=torch.float32):
    return golden_inputs(SHAPE, SEED + 1, dtype)


def main():
    import_reference()
    import dmb.modeling.stereo.disp_refinement.AnyNet as ref_refinement
    from dmb.modeling import build_model

    class SPN(torch.nn.Module):
        def __init__(self, horizontal, reverse):
            super().__init__()
            self.horizontal, self.reverse = horizontal, reverse

        def forward(self, X, G1, G2, G3):
            return O.spn_gaterecurrent2d(X, G1, G2, G3, self.horizontal, self.reverse)

    ref_refinement.GateRecurrent2dnoind = SPN
    # the reference pins its samples to FP32 (cost_processors/AnyNet.py:62 ``.float()``), which grid_sample refuses next to FP64
    # features: the FP64 forward takes them in the features' dtype (a no-op in FP32)
    import dmb.modeling.stereo.cost_processors.AnyNet as ref_proc
    dif = ref_proc.fast_dif_fms
    ref_proc.fast_dif_fms = lambda left, right, disp_sample: dif(left, right, disp_sample=disp_sample.to(left.dtype))
    torch.set_num_threads(8)
    cfg = load_cfg('configs/AnyNet/scene_flow.py')
    model = build_model(cfg)
    sd = seeded_state(model)
    model.load_state_dict(sd, strict=True)
    model.eval()
    out = {}
    out['sd_names'] = np.array(list(sd.keys()))
    out['sd_shapes'] = np.array([','.join(str(s) for s in v.shape) for v in sd.values()])
    out['sd_dtypes'] = np.array([str(v.dtype).replace('torch.', '') for v in sd.values()])
    for k, v in sd.items():
        if v.dtype == torch.float32:
            out['w/' + k] = v.numpy()
    for dtype, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
        m = model.to(dtype)
        trace = {}

        def hook(name):
            def fn(mod, args, kwargs, res):
                trace.setdefault(name, []).append((args, kwargs, res))
            return fn
        hs = [m.backbone.register_forward_hook(hook('backbone'), with_kwargs=True),
              m.cost_processor.register_forward_hook(hook('proc'), with_kwargs=True),
              m.disp_refinement.register_forward_hook(hook('refine'), with_kwargs=True)]
        for st in m.stage:
            hs.append(m.disp_predictor[st].register_forward_hook(hook('pred_' + st), with_kwargs=True))
        left, right = inputs(dtype)
        with torch.no_grad():
            res, _ = m(dict(leftImage=left, rightImage=right))
        for h in hs:
            h.remove()
        (_, _, (fl, fr)), = trace['backbone']
        for i, s in enumerate((16, 8, 4)):
            out['%s/fms_left_%d' % (tag, s)] = fl[i].numpy()
            out['%s/fms_right_%d' % (tag, s)] = fr[i].numpy()
        procs = {kw['stage']: (kw, r) for _, kw, r in trace['proc']}
        out[tag + '/cost_init'] = procs['init_guess'][1][0].numpy()
        out[tag + '/cost_w8'] = procs['warp_level_8'][1][0].numpy()
        out[tag + '/cost_w4'] = procs['warp_level_4'][1][0].numpy()
        out[tag + '/disp_init'] = trace['pred_init_guess'][0][2].numpy()
        out[tag + '/res_w8'] = trace['pred_warp_level_8'][0][2].numpy()
        out[tag + '/res_w4'] = trace['pred_warp_level_4'][0][2].numpy()
        out[tag + '/disp_w8'] = procs['warp_level_4'][0]['disp'].numpy()
        (_, _, rdisps), = trace['refine']
        out[tag + '/refined'] = rdisps[0].numpy()
        out[tag + '/disp_w4'] = rdisps[1].numpy()
        # the 4 full-resolution maps (the 3 residual maps are their differences)
        out[tag + '/disps'] = torch.stack(res['disps'][:4]).float().numpy() if tag == 'f32' else np.zeros(0)
        assert len(res['disps']) == 7 and len(res['costs']) == 3
    model.float()
    path = os.path.join(ROOT, 'tests', 'golden', 'anynet.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
