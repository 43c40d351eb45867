"""Functional torch restatement of the reference's AnyNet eval forward (dmb/modeling/stereo/models/AnyNet.py and the modules it
builds), written from the reference's semantics with ``F.conv2d`` / ``F.batch_norm`` / ... on a ``state_dict``, in the reference's
operation order.  It is the yardstick of tests/test_anynet_gpu.py at any size, in FP32 and FP64, and scripts/bench_anynet.py's
stock-PyTorch comparison; tests/test_anynet_host.py pins it to tests/golden/anynet.npz (the real reference, recorded by
scripts/gen_golden_anynet.py).  ``spn`` is the scan: the oracle's Python-loop restatement by default (the reference's op is
CUDA-only), or any function with the signature of dmb.ops GateRecurrent2dnoind's forward."""
import torch
import torch.nn.functional as F

STAGES = ('init_guess', 'warp_level_8', 'warp_level_4')
GOLDEN_SHAPE, GOLDEN_SEED = (2, 3, 64, 128), 1235      # scripts/gen_golden_anynet.py: SHAPE, SEED + 1


def golden_inputs(shape=GOLDEN_SHAPE, seed=GOLDEN_SEED, dtype=torch.float32):
    """A seeded image pair: the right view is the left one shifted by 3 columns plus noise."""
    g = torch.Generator().manual_seed(seed)
    left = torch.randn(shape, generator=g)
    right = torch.roll(left, shifts=-3, dims=3) + 0.1 * torch.randn(shape, generator=g)
    return left.to(dtype), right.to(dtype)


def _spn_default(X, G1, G2, G3):
    from oracle import dmb_oracle as O
    return O.spn_gaterecurrent2d(X, G1, G2, G3, True, False)


def _bn(x, sd, p):
    """nn.BatchNorm2d/3d in eval (layers/basic_layers.py:125,183)."""
    return F.batch_norm(x, sd[p + 'running_mean'], sd[p + 'running_var'], sd[p + 'weight'], sd[p + 'bias'], False, 0.0, 1e-5)


def _conv(x, sd, p, stride=1):
    conv = F.conv3d if x.dim() == 5 else F.conv2d
    return conv(x, sd[p + 'weight'], sd.get(p + 'bias'), stride, 1, 1)


def bn_relu_conv(x, sd, p, batch_norm=True, stride=1):
    """layers/basic_layers.py:122-138 / 180-197: [BN] -> ReLU -> Conv; keys p0.* / p2.* (p0 = ReLU, p1.* = Conv without BN)."""
    if batch_norm:
        return _conv(F.relu(_bn(x, sd, p + '0.')), sd, p + '2.', stride)
    return _conv(F.relu(x), sd, p + '1.', stride)


def conv_bn_relu(x, sd, p, batch_norm=True):
    """layers/basic_layers.py:102-119."""
    x = _conv(x, sd, p + '0.')
    return F.relu(_bn(x, sd, p + '1.') if batch_norm else x)


def backbone(img, sd, block_num=2, batch_norm=True):
    """backbones/AnyNet.py:39-98 for one view: [fms_16, fms_mix_8, fms_mix_4]."""
    def down(x, p):                                                   # :58-66
        x = F.max_pool2d(x, 2, 2)
        for i in range(block_num):
            x = bn_relu_conv(x, sd, '%s%d.' % (p, i + 1), batch_norm)
        return x
    x = _conv(img, sd, 'backbone.conv_4x.0.')                         # :40
    x = bn_relu_conv(x, sd, 'backbone.conv_4x.1.', batch_norm, stride=2)
    out_4x = down(x, 'backbone.conv_4x.2.')
    out_8x = down(out_4x, 'backbone.conv_8x.')
    out_16x = down(out_8x, 'backbone.conv_16x.')
    up16 = F.interpolate(out_16x, size=out_8x.shape[-2:], mode='bilinear', align_corners=False)       # :88
    x = torch.cat((out_8x, up16), dim=1)
    mix8 = bn_relu_conv(bn_relu_conv(x, sd, 'backbone.conv_mix_8x.0.', batch_norm), sd, 'backbone.conv_mix_8x.1.', batch_norm)
    up8 = F.interpolate(mix8, size=out_4x.shape[-2:], mode='bilinear', align_corners=False)           # :94
    x = torch.cat((out_4x, up8), dim=1)
    mix4 = bn_relu_conv(bn_relu_conv(x, sd, 'backbone.conv_mix_4x.0.', batch_norm), sd, 'backbone.conv_mix_4x.1.', batch_norm)
    return [out_16x, mix8, mix4]


def fast_dif_fms(left, right, disp_sample):
    """cost_processors/utils/dif_fms.py:49-86 with layers/inverse_warp_3d.py:4-56 (normalize=False)."""
    B, C, H, W = left.shape
    D = disp_sample.shape[1]
    disp_sample = disp_sample.to(left.dtype)     # FP32 samples (cost_processors/AnyNet.py:62) next to FP64 features: FP64
    ref = left.unsqueeze(2).expand(B, C, D, H, W)
    tgt = right.unsqueeze(2).expand(B, C, D, H, W)
    dev = left.device
    grid_d = torch.linspace(0, D - 1, D).view(1, D, 1, 1).expand(B, D, H, W).to(dev)
    grid_h = torch.linspace(0, H - 1, H).view(1, 1, H, 1).expand(B, D, H, W).to(dev)
    grid_w = torch.linspace(0, W - 1, W).view(1, 1, 1, W).expand(B, D, H, W).to(dev)
    grid_w = grid_w + (-disp_sample)
    grid_d = (grid_d / (D - 1) * 2) - 1
    grid_h = (grid_h / (H - 1) * 2) - 1
    grid_w = (grid_w / (W - 1) * 2) - 1
    grid = torch.cat((grid_w.unsqueeze(4), grid_h.unsqueeze(4), grid_d.unsqueeze(4)), 4)
    tgt = F.grid_sample(tgt, grid, padding_mode='zeros')
    ref = ref * (tgt > 0).type_as(ref)
    return ref - tgt


def aggregate(raw, sd, stage, num=4, batch_norm=True):
    """cost_processors/aggregators/AnyNet.py:29-50."""
    x = raw
    for i in range(num + 2):
        x = bn_relu_conv(x, sd, 'cost_processor.aggregator.%s.agg.%d.' % (stage, i), batch_norm)
    return x.squeeze(dim=1)


def processor(left, right, stage, sd, cfg, disp=None, batch_norm=True):
    """cost_processors/AnyNet.py:49-79: (cost [B, D, H, W], samples)."""
    cc = cfg['cost_computation']
    B, C, H, W = left.shape
    start, md, dil = cc['start_disp'][stage], cc['max_disp'][stage], cc['dilation'][stage]
    D = (md + dil - 1) // dil
    sample = torch.linspace(start, start + md - 1, D).view(1, D, 1, 1).expand(B, D, H, W).to(left.device).float()
    if disp is not None:
        scale = W / disp.shape[-1]
        disp = F.interpolate(disp * scale, size=(H, W), mode='bilinear', align_corners=False)
        sample = sample + disp
    raw = fast_dif_fms(left, right, sample)
    return aggregate(raw, sd, stage, batch_norm=batch_norm), sample


def regress(cost, sd, stage, alpha=1.0):
    """disp_predictors/faster_soft_argmin.py:51-75 (normalize=True)."""
    prob = F.softmax(cost * alpha, dim=1).unsqueeze(1)
    return F.conv3d(prob, sd['disp_predictor.%s.disp_regression.weight' % stage].to(cost.dtype)).squeeze(1)


def refinement(init_disp, left_img, sd, spn=None, spn_planes=8, batch_norm=True):
    """disp_refinement/AnyNet.py:57-98: the refined map."""
    spn = spn or _spn_default
    h, w = init_disp.shape[-2:]
    img = F.interpolate(left_img, size=(h, w), mode='bilinear', align_corners=False)
    G = img
    for i in range(3):
        G = conv_bn_relu(G, sd, 'disp_refinement.img_conv.%d.' % i, batch_norm)
    G = _conv(G, sd, 'disp_refinement.img_conv.3.')
    G1, G2, G3 = torch.split(G, spn_planes, dim=1)
    sum_abs = G1.abs() + G2.abs() + G3.abs()
    G1, G2, G3 = (torch.div(g, sum_abs + 1e-8) for g in (G1, G2, G3))
    feat = _conv(init_disp, sd, 'disp_refinement.disp_conv.')
    prop = spn(feat, G1, G2, G3)
    res = _conv(prop, sd, 'disp_refinement.classify.')
    return F.relu(res + init_disp)


def combine(low, high):
    """models/AnyNet.py:80-85."""
    H, W = high.shape[-2:]
    scale = W / low.shape[-1]
    return F.interpolate(low * scale, size=(H, W), mode='bilinear', align_corners=False) + high


def forward(left_img, right_img, sd, cfg, spn=None, batch_norm=True, trace=None):
    """models/AnyNet.py:43-147 (eval).  ``cfg``: the model's cost_processor dict.  Returns (disps [7], costs [3]); ``trace`` (a
    dict) receives the stage-boundary tensors."""
    t = trace if trace is not None else {}
    fl, fr = backbone(left_img, sd, batch_norm=batch_norm), backbone(right_img, sd, batch_norm=batch_norm)
    t['fms_left'], t['fms_right'] = fl, fr
    c_init, _ = processor(fl[0], fr[0], 'init_guess', sd, cfg, None, batch_norm)
    d_init = regress(c_init, sd, 'init_guess')
    c8, _ = processor(fl[1], fr[1], 'warp_level_8', sd, cfg, d_init, batch_norm)
    r8 = regress(c8, sd, 'warp_level_8')
    d8 = combine(d_init, r8)
    c4, _ = processor(fl[2], fr[2], 'warp_level_4', sd, cfg, d8, batch_norm)
    r4 = regress(c4, sd, 'warp_level_4')
    d4 = combine(d8, r4)
    refined = refinement(d4, left_img, sd, spn, batch_norm=batch_norm)
    t.update(cost_init=c_init, disp_init=d_init, cost_w8=c8, res_w8=r8, disp_w8=d8, cost_w4=c4, res_w4=r4, disp_w4=d4,
             refined=refined)
    H, W = left_img.shape[-2:]
    disps = [F.interpolate(d * W / d.shape[-1], size=(H, W), mode='bilinear', align_corners=False)
             for d in (refined, d4, d8, d_init)]
    disps = disps + [disps[i - 1] - disps[i] for i in range(1, 4)]
    return disps, [c4, c8, c_init]
