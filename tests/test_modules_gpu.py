"""The drop-in modules (reference API surface) on the GPU against (a) golden vectors produced by the real
reference and (b) the CPU oracle on the same seeded inputs; plus full-size (BASELINE cfg2) property tests."""
import os

import numpy as np
import pytest
import torch

from oracle import dmb_oracle as O
from tests._util import golden, maxdiff, rand, sha

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DISP_TOL = 1e-4   # north-star: max abs on the disparity map
COST_TOL = 5e-5   # costs are O(1..10) after 25+ FP32 conv layers in a different summation order


def _load(module, params, prefix=""):
    sd = {prefix + k: v for k, v in params.items()}
    missing, unexpected = module.load_state_dict(sd, strict=False)
    missing = [k for k in missing if k.startswith(prefix) and not k.endswith("num_batches_tracked")]
    assert not unexpected and not missing, (missing, unexpected)
    return module


def test_psm_aggregator_vs_reference_golden(dev):
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.aggregators import PSMAggregator
    from densematchingbenchmark_amd.modeling.stereo.disp_predictors import PREDICTORS
    g = golden("aggregators.npz")
    raw = rand((1, 64, 8, 16, 32), 301)
    p = O.random_params_psm(seed=0, classif_gain=10.0)
    m = _load(PSMAggregator(max_disp=32, in_planes=64, batch_norm=True), p).eval().to(dev)
    pred = PREDICTORS['FASTER'](max_disp=32).to(dev)
    with torch.no_grad():
        costs = m(raw.to(dev))
        for c, k in zip(costs, ("psm_cost3", "psm_cost2", "psm_cost1")):
            assert maxdiff(c[:, ::4, ::8, :], g[k]) <= COST_TOL
        for c, k in zip(costs, ("psm_disp3", "psm_disp2", "psm_disp1")):
            assert maxdiff(pred(c), g[k]) <= DISP_TOL
        # hourglass cross links
        c0 = m.dres0(raw.to(dev))
        c0 = m.dres1[1](m.dres1[0](c0), residual=c0)
        o1, pre1, post1 = m.dres2(c0, None, None)
        assert maxdiff(o1[:, ::8], g["hg_out"]) <= COST_TOL and maxdiff(pre1[:, ::16], g["hg_pre"]) <= COST_TOL
        assert maxdiff(post1[:, ::16], g["hg_post"]) <= COST_TOL
        o2, pre2, post2 = m.dres3(o1 + c0, pre1, post1)
        assert maxdiff(o2[:, ::8], g["hg2_out"]) <= COST_TOL and maxdiff(post2[:, ::16], g["hg2_post"]) <= COST_TOL
        # full tensors against the oracle
        ref = O.psm_aggregator(raw, p, 32)
        for a, b in zip(costs, ref):
            assert maxdiff(a, b) <= COST_TOL


def test_acf_aggregator_and_conf_heads(dev):
    from densematchingbenchmark_amd.modeling.stereo.cmn import ConfHead
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.aggregators import AGGREGATORS
    g = golden("aggregators.npz")
    raw = rand((1, 64, 8, 16, 32), 301)
    p = O.random_params_psm(seed=1, classif_gain=10.0, acf=True)
    m = _load(AGGREGATORS["AcfNet"](max_disp=32, in_planes=64, batch_norm=True), p).eval().to(dev)
    with torch.no_grad():
        costs = m(raw.to(dev))
        for c, k in zip(costs, ("acf_cost3", "acf_cost2", "acf_cost1")):
            assert maxdiff(c[:, ::4, ::8, :], g[k]) <= COST_TOL
        for i, c in enumerate(costs):
            head = ConfHead(32, batch_norm=True).eval()
            hp = {k[len("confp_%d_" % i):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("confp_%d_" % i)}
            _load(head, hp)
            conf = head.to(dev)(c)
            assert maxdiff(conf, g["conf_%d" % i]) <= 1e-5


def test_stereonet_aggregator(dev):
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.aggregators import AGGREGATORS
    g = golden("aggregators.npz")
    sp = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("snp_")}
    m = _load(AGGREGATORS["StereoNet"](max_disp=48, in_planes=32, batch_norm=True, num=4), sp).eval().to(dev)
    with torch.no_grad():
        cost = m(rand((2, 32, 6, 10, 20), 302).to(dev))[0]
    assert maxdiff(cost, g["sn_cost"]) <= 2e-5


def test_psmnet_path_cfg1_through_builders(dev):
    """BASELINE configs[0]: PSMNet cat volume + soft-argmin, 256x512, max_disp=64, via build_model(cfg, backbone=None)."""
    from densematchingbenchmark_amd.config import Config
    from densematchingbenchmark_amd.modeling import build_model
    g = golden("psmnet_path_cfg1.npz")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "PSMNet", "scene_flow.py"))
    md = 64
    cfg.model.max_disp = md
    cfg.model.cost_processor.cost_computation.max_disp = md // 4
    cfg.model.cost_processor.cost_aggregator.max_disp = md
    cfg.model.disp_predictor.max_disp = md
    model = build_model(cfg, backbone=None).eval()
    assert sorted(k for k in model.cost_processor.state_dict()) == [str(s) for s in g["cp_keys"]]
    assert sorted(k for k in model.disp_predictor.state_dict()) == [str(s) for s in g["disp_keys"]]
    _load(model, O.random_params_psm(seed=2, classif_gain=10.0), "cost_processor.aggregator.")
    model = model.to(dev)
    lf, rf = rand((1, 32, 64, 128), 401), rand((1, 32, 64, 128), 402)
    results, losses = model(dict(leftFeature=lf.to(dev), rightFeature=rf.to(dev)))
    assert losses == {} and set(results) == {"disps", "costs"} and len(results["disps"]) == 3
    for i, (d, c) in enumerate(zip(results["disps"], results["costs"])):
        assert d.shape == (1, 1, 256, 512) and c.shape == (1, 64, 256, 512)
        assert maxdiff(d[:, :, ::2, ::2], g["disp%d" % (3 - i)]) <= DISP_TOL
        assert maxdiff(c[:, ::8, ::32, :], g["cost%d_rows" % (3 - i)]) <= COST_TOL


def test_branch_overlap_is_identical(dev):
    """ops.set_branch_overlap: the classifier branches on a second stream next to the following hourglass -- same kernels, same
    operands, so every output is bit-identical to the sequential issue order (twice: the second call reuses the stream)."""
    from densematchingbenchmark_amd import ops
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.aggregators import PSMAggregator
    m = _load(PSMAggregator(max_disp=32, in_planes=64), O.random_params_psm(seed=6, classif_gain=10.0)).to(dev).eval()
    raw = rand((2, 64, 8, 16, 32), 305).to(dev)
    with torch.no_grad():
        want = m(raw)
        ops.set_branch_overlap(True)
        try:
            for _ in range(2):
                got = m(raw)
                torch.cuda.synchronize()
                for a, b in zip(got, want):
                    assert torch.equal(a, b)
                    vals = ops.disp_sample_values(32, 0, 1)
                    ha, hb = ops.RegressionHint.lookup(a, vals, 1.0, True), ops.RegressionHint.lookup(b, vals, 1.0, True)
                    assert ha is not None and torch.equal(ha, hb)
        finally:
            ops.set_branch_overlap(False)


def test_fast_mode_cost_processor_through_builders(dev):
    """cost_computation.type='fast_mode' (the AnyNet config's builder, configs/AnyNet/scene_flow.py:34-35) through
    build_cost_processor: the warped volume feeds the same aggregator; with and without explicit per-pixel samples."""
    from densematchingbenchmark_amd.config import Config
    from densematchingbenchmark_amd.modeling.stereo.cost_processors import build_cost_processor
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "PSMNet", "scene_flow.py"))
    md = 32
    cfg.model.max_disp = md
    cfg.model.cost_processor.cost_computation.max_disp = md // 4
    cfg.model.cost_processor.cost_computation.type = "fast_mode"
    cfg.model.cost_processor.cost_aggregator.max_disp = md
    cp = build_cost_processor(cfg).eval()
    p = O.random_params_psm(seed=4, classif_gain=10.0)
    _load(cp, p, "aggregator.")
    cp = cp.to(dev)
    lf, rf = rand((1, 32, 16, 32), 411), rand((1, 32, 16, 32), 412)
    with torch.no_grad():
        for ds in (None, (torch.arange(8.0).view(1, 8, 1, 1) + rand((1, 8, 16, 32), 413, 0.3))):
            costs = cp(lf.to(dev), rf.to(dev), disp_sample=None if ds is None else ds.to(dev))
            raw = O.fast_cat_fms(lf, rf, md // 4, 0, 1, disp_sample=ds)
            want = O.psm_aggregator(raw, p, md)
            for a, b in zip(costs, want):
                assert maxdiff(a, b) <= COST_TOL


def test_predictor_modules_vs_golden(dev):
    from densematchingbenchmark_amd.modeling.stereo.disp_predictors import PREDICTORS
    g = golden("predictors.npz")
    for tag in ("flat", "peaked", "d192"):
        D, seed = (int(v) for v in g[tag + "_meta"])
        cost = rand((2, D, 6, 10), seed, float(g[tag + "_gain"][0])).to(dev)
        kw = dict(max_disp=D, start_disp=0, dilation=1, alpha=1.0, normalize=True)
        tol = 1.5e-4 if tag == "flat" or D == 192 else DISP_TOL   # flat / wide: the reference's own FP32 floor
        assert maxdiff(PREDICTORS['DEFAULT'](**kw)(cost), g[tag + "_soft"]) <= tol
        assert maxdiff(PREDICTORS['FASTER'](**kw).to(dev)(cost), g[tag + "_faster"]) <= tol
        disp, idx = PREDICTORS['LOCAL'](radius=2, **kw)(cost, return_index=True)
        assert np.array_equal(idx.cpu().numpy(), g[tag + "_argmax"])     # bit-exact index path
        assert maxdiff(disp, g[tag + "_local"]) <= DISP_TOL
    cost = rand((1, 12, 4, 6), 204, 5.0).to(dev)
    assert maxdiff(PREDICTORS['DEFAULT'](24, -6, 2, 0.7)(cost), g["dil_soft"]) <= 1e-5
    assert maxdiff(PREDICTORS['LOCAL'](24, 3, -6, 2, 2, 0.7)(cost), g["dil_local"]) <= 1e-5
    assert maxdiff(PREDICTORS['DEFAULT'](12, 0, 1, 0.5, False)(cost), g["nonorm_soft"]) <= 1e-4
    samp = rand((1, 12, 4, 6), 205, 10.0).to(dev)
    assert maxdiff(PREDICTORS['DEFAULT'](12)(cost, samp), g["sampled_soft"]) <= 1e-5


def test_volume_funcs_vs_golden(dev):
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils.cat_fms import CAT_FUNCS
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils.dif_fms import DIF_FUNCS
    g = golden("volumes.npz")
    for i, row in enumerate(g["cases"]):
        shape, (md, sd, dil, seed) = tuple(int(v) for v in row[:4]), (int(v) for v in row[4:])
        a, b = rand(shape, seed).to(dev), rand(shape, seed + 1000).to(dev)
        assert sha(CAT_FUNCS['default'](a, b, max_disp=md, start_disp=sd, dilation=dil)) == str(g["cat_sha_%d" % i])
        assert sha(DIF_FUNCS['default'](a, b, max_disp=md, start_disp=sd, dilation=dil)) == str(g["dif_sha_%d" % i])


def test_gwc_cat_volume_feeds_psm_aggregator(dev):
    """BASELINE configs[2] wiring (no reference implementation -> parity unpinned, oracle = spec)."""
    from densematchingbenchmark_amd.config import Config
    from densematchingbenchmark_amd.modeling.stereo.cost_processors import build_cost_processor
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "GwcNet", "scene_flow.py"))
    cfg.model.cost_processor.cost_computation.max_disp = 8
    cfg.model.cost_processor.cost_aggregator.max_disp = 32
    cp = build_cost_processor(cfg).eval().to(dev)
    lg, rg = rand((1, 320, 16, 32), 601), rand((1, 320, 16, 32), 602)
    lc, rc = rand((1, 12, 16, 32), 603), rand((1, 12, 16, 32), 604)
    vol = cp.vol_func((lg.to(dev), lc.to(dev)), (rg.to(dev), rc.to(dev)), **cp.default_args)
    assert vol.shape == (1, 64, 8, 16, 32)
    assert maxdiff(vol[:, :40], O.gwc_fms(lg, rg, 8, 0, 1, 40)) <= 3e-6
    assert torch.equal(vol[:, 40:].cpu(), O.cat_fms(lc, rc, 8, 0, 1))
    costs = cp.aggregator(vol)
    assert len(costs) == 3 and costs[0].shape == (1, 32, 64, 128)


def test_eval_accumulator_matches_reference_semantics(dev):
    from densematchingbenchmark_amd.evaluation import EpeAccumulator, calc_error
    g = golden("evaluation.npz")
    gen = torch.Generator().manual_seed(501)
    gt = torch.rand((3, 1, 20, 32), generator=gen) * 220 - 10
    est = gt + torch.randn((3, 1, 20, 32), generator=gen) * 3
    gt[2] = -1.0
    acc = EpeAccumulator(dev, 1, 0, 192)
    acc.update([est.to(dev)], gt.to(dev), (17, 30))
    got = acc.all_reduce().summary()[0]
    want = np.mean([g["img%d" % b] for b in range(3)], axis=0)
    for j, k in enumerate(("epe", "1px", "2px", "3px", "5px")):
        assert abs(got[k] - want[j]) <= 1e-5 * max(1.0, abs(want[j]))
    e = calc_error(est[0, 0, 3:, :30].to(dev), gt[0, 0, 3:, :30].to(dev), 0, 192)
    assert abs(e["epe"] - g["img0"][0]) <= 1e-5


# ------------------------------------------------------------------------------------------- full size (cfg2)
FULL = dict(D=48, H=136, W=240)


def test_full_size_conv_is_exactly_linear_and_shift_equivariant(dev):
    """Size-independent properties at the BASELINE cfg2 volume size: an FP32 fma chain commutes with scaling by a
    power of two bit-exactly, and a 3x3x3 convolution is translation equivariant away from the borders."""
    from densematchingbenchmark_amd import ops
    x = rand((1, 32, FULL["D"], FULL["H"], FULL["W"]), 701).to(dev)
    w = rand((32, 32, 3, 3, 3), 702, 0.03).to(dev)
    wp = ops.pack_conv3d_weights(w)
    y = ops.conv3d_k3(x, wp, 32)
    assert torch.equal(ops.conv3d_k3(x * 4.0, wp, 32), y * 4.0)
    xs = torch.roll(x, shifts=(1, 2, 3), dims=(2, 3, 4))
    ys = ops.conv3d_k3(xs, wp, 32)
    assert torch.equal(ys[:, :, 3:-3, 4:-4, 5:-5], torch.roll(y, shifts=(1, 2, 3), dims=(2, 3, 4))[:, :, 3:-3, 4:-4, 5:-5])
    # one full-size layer against the oracle primitive (about a second of CPU)
    ref = torch.nn.functional.conv3d(x.cpu(), w.cpu(), None, padding=1)
    assert maxdiff(y, ref) <= 2e-5


def test_full_size_volume_and_regression_properties(dev):
    from densematchingbenchmark_amd import ops
    L = rand((1, 32, FULL["H"], FULL["W"]), 703).to(dev)
    R = rand((1, 32, FULL["H"], FULL["W"]), 704).to(dev)
    idx = ops.disp_index_list(48, 0, 1)
    vol = ops.cat_fms(L, R, idx)
    # checksum of checksums: plane k keeps columns x >= k of both features
    for k in (0, 1, 17, 47):
        assert torch.equal(vol[0, :32, k, :, k:], L[0, :, :, k:]) and torch.equal(vol[0, 32:, k, :, k:], R[0, :, :, :240 - k])
        assert vol[0, :, k, :, :k].abs().sum().item() == 0
    assert torch.equal(ops.dif_fms(L, R, idx)[0, :, 5, :, 5:], L[0, :, :, 5:] - R[0, :, :, :-5])
    # soft-argmin of a sharply one-hot cost returns exactly the sample value; arg-max path returns the index
    cost = torch.zeros((1, 192, 544, 960), device=dev)
    k = torch.randint(0, 192, (1, 1, 544, 960), generator=torch.Generator().manual_seed(705)).to(dev)
    cost.scatter_(1, k, 200.0)
    vals = ops.disp_sample_values(192, 0, 1)
    assert torch.equal(ops.soft_argmin(cost, vals), k.float())
    d, i = ops.local_soft_argmin(cost, 2, return_index=True)
    assert torch.equal(i, k) and torch.equal(d, k.float())
    # trilinear (align_corners) reproduces the corner samples and stays within the input range
    q = rand((1, 48, 136, 240), 706).to(dev)
    up = ops.trilinear_ac(q, (192, 544, 960))
    assert torch.equal(up[0, 0, 0, 0], q[0, 0, 0, 0]) and torch.equal(up[0, -1, -1, -1], q[0, -1, -1, -1])
    assert up.max() <= q.max() + 1e-6 and up.min() >= q.min() - 1e-6
    # fused up-sampling + regression: bit-identical logits (same lerp order, same alpha scaling); only the online
    # soft-max regrouping differs -> a few ulp of the disparity
    assert maxdiff(ops.trilinear_soft_argmin(q, (192, 544, 960), vals, 3.0), ops.soft_argmin(up, vals, 3.0)) <= 1e-4


# (the full-size FP64-yardstick tests -- every pair of the bench batch, AcfNet, GwcNet, classifier gain 30 -- live in
#  tests/test_fullsize_gpu.py)


def _built(cfg_rel, seed, tweak=None):
    from densematchingbenchmark_amd import synthetic
    from densematchingbenchmark_amd.config import Config
    from densematchingbenchmark_amd.modeling import build_model
    cfg = Config.fromfile(os.path.join(ROOT, "configs", cfg_rel))
    if tweak:
        tweak(cfg)
    model = build_model(cfg, backbone=None).eval()
    synthetic.init_params_(model, seed=seed, classif_gain=10.0)
    return cfg, model


def _acf32(cfg):
    cfg.model.max_disp = 32
    cfg.model.cost_processor.cost_computation.max_disp = 8
    cfg.model.cost_processor.cost_aggregator.max_disp = 32
    cfg.model.disp_predictor.max_disp = 32
    cfg.model.cmn.in_planes = 32


def test_acfnet_model_vs_reference_golden(dev):
    """BASELINE configs[3] wiring: cat volume -> AcfAggregator (learned k8/s4 up-sampling) -> soft-argmin + Cmn
    confidences, against outputs of the reference's own build_cost_processor / Cmn on the same parameters."""
    g = golden("acfnet_path.npz")
    cfg, model = _built("AcfNet/scene_flow_adaptive.py", 5, _acf32)
    model = model.to(dev)
    lf, rf = rand((2, 32, 16, 32), 411), rand((2, 32, 16, 32), 412)
    results, _ = model(dict(leftFeature=lf.to(dev), rightFeature=rf.to(dev)))
    assert set(results) == {"disps", "costs", "confs"}
    for i in range(3):
        assert maxdiff(results["disps"][i], g["disp%d" % (3 - i)]) <= DISP_TOL
        assert maxdiff(results["confs"][i], g["conf%d" % (3 - i)]) <= 1e-5
        assert maxdiff(results["costs"][i][:, ::4, ::8, :], g["cost%d_rows" % (3 - i)]) <= COST_TOL
    with torch.no_grad():
        variance, confs = model.cmn(results["costs"])
    assert maxdiff(variance[0], g["var3"]) <= 1e-5


def test_stereonet_model_vs_reference_golden(dev):
    """BASELINE configs[4] wiring: dif volume at 1/8 -> StereoNetAggregator -> soft-argmin over 24 samples."""
    g = golden("stereonet_path.npz")
    cfg, model = _built("StereoNet/scene_flow_8x_2stage.py", 6)
    model = model.to(dev)
    lf, rf = rand((2, 32, 20, 36), 421), rand((2, 32, 20, 36), 422)
    results, _ = model(dict(leftFeature=lf.to(dev), rightFeature=rf.to(dev)))
    assert len(results["disps"]) == 1
    assert maxdiff(results["costs"][0], g["cost"]) <= 2e-5 and maxdiff(results["disps"][0], g["disp"]) <= DISP_TOL


def test_gwcnet_model_vs_oracle(dev):
    """BASELINE configs[2]: no reference implementation exists (parity UNPINNED) -- the oracle states the spec."""
    def tweak(cfg):
        cfg.model.max_disp = 32
        cfg.model.cost_processor.cost_computation.max_disp = 8
        cfg.model.cost_processor.cost_aggregator.max_disp = 32
        cfg.model.disp_predictor.max_disp = 32
    cfg, model = _built("GwcNet/scene_flow.py", 7, tweak)
    p = {k: v.clone() for k, v in model.state_dict().items()}
    lg, rg = rand((1, 320, 16, 32), 431), rand((1, 320, 16, 32), 432)
    lc, rc = rand((1, 12, 16, 32), 433), rand((1, 12, 16, 32), 434)
    model = model.to(dev)
    results, _ = model(dict(leftFeature=(lg.to(dev), lc.to(dev)), rightFeature=(rg.to(dev), rc.to(dev))))
    disps, costs = O.gwcnet_path((lg, lc), (rg, rc), p, 32)
    for a, b in zip(results["disps"], disps):
        assert maxdiff(a, b) <= DISP_TOL
    for a, b in zip(results["costs"], costs):
        assert maxdiff(a, b) <= COST_TOL


# -------------------------------------------------------------------------------- "next" row: PSMNet backbone (8-f1)
def test_psmnet_backbone_vs_reference_golden(dev):
    from densematchingbenchmark_amd import synthetic
    from densematchingbenchmark_amd.modeling.stereo.backbones import PSMNetBackbone
    g = golden("psmnet_backbone.npz")
    bb = PSMNetBackbone(3, True).eval()
    synthetic.init_params_(bb, seed=8, classif_gain=1.0)
    bb = bb.to(dev)
    img = rand((1, 3, 256, 512), 441)
    with torch.no_grad():
        fl, fr = bb(img.to(dev), rand((1, 3, 256, 512), 442).to(dev))
    assert fl.shape == (1, 32, 64, 128)
    assert maxdiff(fl[:, :, ::2, ::2], g["feat"]) <= 5e-6          # features are O(0.1..1) after 50+ FP32 conv layers
    p = {"backbone." + k: v.cpu() for k, v in bb.state_dict().items()}
    assert maxdiff(fr, O.psmnet_backbone(rand((1, 3, 256, 512), 442), p)) <= 5e-6   # second view through the 2B batch
    # odd sizes: H/4, W/4 not multiples of the pooling windows' tiles
    img = rand((2, 3, 256, 328), 443)
    with torch.no_grad():
        fl, _ = bb(img.to(dev), img.to(dev))
    assert maxdiff(fl, O.psmnet_backbone(img, p)) <= 5e-6


def test_psmnet_end_to_end_vs_reference_golden(dev):
    """Images -> backbone -> cost volume -> hourglass -> soft-argmin, against the reference's whole model."""
    from densematchingbenchmark_amd import synthetic
    from densematchingbenchmark_amd.config import Config
    from densematchingbenchmark_amd.modeling import build_model
    g = golden("psmnet_e2e_cfg1.npz")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "PSMNet", "scene_flow.py"))
    cfg.model.max_disp = 64
    cfg.model.cost_processor.cost_computation.max_disp = 16
    cfg.model.cost_processor.cost_aggregator.max_disp = 64
    cfg.model.disp_predictor.max_disp = 64
    cfg.model.backbone = dict(type="PSMNet", in_planes=3)
    model = build_model(cfg, backbone="hip").eval()
    synthetic.init_params_(model, seed=9, classif_gain=10.0)
    model = model.to(dev)
    batch = {"leftImage": rand((1, 3, 256, 512), 451).to(dev), "rightImage": rand((1, 3, 256, 512), 452).to(dev)}
    with torch.no_grad():
        result, _ = model(batch)
    for i, d in enumerate(result["disps"]):
        assert maxdiff(d[:, :, ::2, ::2], g["disp%d" % (3 - i)]) <= DISP_TOL


# ----------------------------------------------------------------- "next" row: StereoNet edge-aware refinement (8-f2)
def test_stereonet_refinement_vs_reference_golden(dev):
    from densematchingbenchmark_amd import synthetic
    from densematchingbenchmark_amd.modeling.stereo.disp_refinement import StereoNetRefinement
    g = golden("stereonet_refinement.npz")
    rf = StereoNetRefinement(in_planes=4, batch_norm=True, num=2).eval()
    synthetic.init_params_(rf, seed=10, classif_gain=1.0)
    rf = rf.to(dev)
    gen = torch.Generator().manual_seed(461)
    coarse = torch.rand((2, 1, 24, 40), generator=gen) * 4.0
    with torch.no_grad():
        outs = rf([coarse.to(dev)], None, None, rand((2, 3, 192, 320), 462).to(dev), None)
    assert len(outs) == 3 and outs[0].shape == (2, 1, 192, 320)
    for i, d in enumerate(outs):
        assert maxdiff(d[:, :, ::2, ::2], g["refined%d" % i]) <= DISP_TOL


def test_stereonet_model_with_refinement_vs_oracle(dev):
    """The whole StereoNet-8x model after the backbone (config #5 at a reduced size): difference volume -> aggregator ->
    soft-argmin at 1/8 -> edge-aware refinement at full resolution, against the CPU oracle on the same inputs."""
    from densematchingbenchmark_amd import synthetic
    from densematchingbenchmark_amd.config import Config
    from densematchingbenchmark_amd.modeling import build_model
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "StereoNet", "scene_flow_8x_2stage.py"))
    cfg.model.disp_refinement = dict(type="StereoNet", in_planes=4, num=1)
    model = build_model(cfg, backbone=None).eval()
    synthetic.init_params_(model, seed=11, classif_gain=10.0)
    p = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    lf, rf = rand((1, 32, 20, 39), 471), rand((1, 32, 20, 39), 472)
    img = rand((1, 3, 160, 312), 473)
    with torch.no_grad():
        res, _ = model(dict(leftFeature=lf.to(dev), rightFeature=rf.to(dev), leftImage=img.to(dev)))
    disps, _ = O.stereonet_path(lf, rf, p, 192)
    want = O.stereonet_refinement(disps, img, p, num=1)
    assert len(res["disps"]) == 2
    for a, b in zip(res["disps"], want):
        assert maxdiff(a, b) <= DISP_TOL


def test_stereonet_end_to_end_vs_reference_golden(dev):
    """Images -> StereoNet backbone -> difference volume -> aggregator -> soft-argmin -> refinement, all HIP, against
    the reference's whole model (config scene_flow_8x_2stage)."""
    from densematchingbenchmark_amd import synthetic
    from densematchingbenchmark_amd.config import Config
    from densematchingbenchmark_amd.modeling import build_model
    g = golden("stereonet_e2e.npz")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "StereoNet", "scene_flow_8x_2stage.py"))
    cfg.model.backbone = dict(type="StereoNet", in_planes=3, downsample_num=3, residual_num=6)
    cfg.model.disp_refinement = dict(type="StereoNet", in_planes=4, num=1)
    model = build_model(cfg, backbone="hip").eval()
    synthetic.init_params_(model, seed=12, classif_gain=10.0)
    model = model.to(dev)
    li, ri = rand((1, 3, 192, 320), 481).to(dev), rand((1, 3, 192, 320), 482).to(dev)
    with torch.no_grad():
        lf, _ = model.backbone(li, ri)
        res, _ = model(dict(leftImage=li, rightImage=ri))
    assert maxdiff(lf, g["left_feature"]) <= 2e-5
    assert len(res["disps"]) == 2
    for i, d in enumerate(res["disps"]):
        assert maxdiff(d, g["disp%d" % i]) <= DISP_TOL


# ------------------------------------------------------------------------------------------ GC-Net
def test_gcnet_aggregator_vs_reference_golden(dev):
    from densematchingbenchmark_amd import synthetic
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.aggregators import GCAggregator
    g = golden("gcnet_aggregator.npz")
    ga = GCAggregator(max_disp=32, in_planes=64, batch_norm=True).eval()
    synthetic.init_params_(ga, seed=13, classif_gain=30.0)
    ga = ga.to(dev)
    with torch.no_grad():
        cost = ga(rand((1, 64, 16, 16, 32), 491).to(dev))[0]
    assert cost.shape == (1, 32, 32, 64)
    assert maxdiff(cost[:, ::2, ::2, ::2], g["cost"]) <= COST_TOL


def test_gcnet_end_to_end_vs_reference_golden(dev):
    from densematchingbenchmark_amd import synthetic
    from densematchingbenchmark_amd.config import Config
    from densematchingbenchmark_amd.modeling import build_model
    g = golden("gcnet_e2e.npz")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "GCNet", "scene_flow.py"))
    cfg.model.max_disp = 64
    cfg.model.cost_processor.cost_computation.max_disp = 32
    cfg.model.cost_processor.cost_aggregator.max_disp = 64
    cfg.model.disp_predictor.max_disp = 64
    model = build_model(cfg, backbone="hip").eval()
    synthetic.init_params_(model, seed=14, classif_gain=30.0)
    model = model.to(dev)
    li, ri = rand((1, 3, 64, 128), 492).to(dev), rand((1, 3, 64, 128), 493).to(dev)
    with torch.no_grad():
        lf, _ = model.backbone(li, ri)
        res, _ = model(dict(leftImage=li, rightImage=ri))
    assert maxdiff(lf[:, ::2], g["left_feature"]) <= 2e-5
    assert len(res["disps"]) == 1 and maxdiff(res["disps"][0], g["disp"]) <= DISP_TOL


# ------------------------------------------------------------------ training-side losses (first part)
def test_losses_forward_backward_vs_reference_golden(dev):
    """Loss values and gradients (d/d cost, d/d variance, d/d confidence logits, d/d disparity) of the HIP kernels under
    torch autograd against the reference's own values and autograd gradients."""
    from densematchingbenchmark_amd.modeling.stereo.losses import ConfidenceNllLoss, DispSmoothL1Loss, StereoFocalLoss
    g = golden("losses.npz")
    gt = torch.from_numpy(g["gt"]).to(dev)
    for tag, coef in (("a", 0.0), ("b", 5.0)):
        cost = (rand((2, 48, 12, 20), 512) * 3.0).to(dev).requires_grad_(True)
        var = torch.from_numpy(g["focal_b_var"]).to(dev).requires_grad_(True) if tag == "b" else 1.2
        loss = StereoFocalLoss(max_disp=48, start_disp=0, dilation=1, weights=(0.7,), focal_coefficient=coef)(
            cost, gt, var)["stereo_focal_loss_lvl0"]
        loss.backward()
        want = g["focal_%s_loss" % tag][0]
        assert abs(float(loss.detach()) - want) <= 2e-5 * abs(want)
        gc = g["focal_%s_gcost" % tag]
        assert maxdiff(cost.grad, gc) <= 2e-5 * np.abs(gc).max()
        if tag == "b":
            assert maxdiff(var.grad, g["focal_b_gvar"]) <= 1e-4 * np.abs(g["focal_b_gvar"]).max()
    conf = (rand((2, 1, 12, 20), 513) * 2.0).to(dev).requires_grad_(True)
    l = ConfidenceNllLoss(max_disp=48, weights=(1.0,))(conf, gt)["conf_loss_lvl0"]
    l.backward()
    assert abs(float(l.detach()) - g["conf_loss"][0]) <= 2e-6 and maxdiff(conf.grad, g["conf_grad"]) <= 1e-8
    est = (torch.from_numpy(g["gt"]) + rand((2, 1, 12, 20), 514) * 2.0).to(dev).requires_grad_(True)
    l = DispSmoothL1Loss(max_disp=48, weights=(1.0,))(est, gt)["l1_loss_lvl0"]
    l.backward()
    assert abs(float(l.detach()) - g["l1_loss"][0]) <= 2e-6 and maxdiff(est.grad, g["l1_grad"]) <= 1e-8


def test_focal_loss_multi_level_and_empty_mask(dev):
    """A half-resolution cost level uses the pooled, rescaled ground truth (stereo_focal_loss.py:66-73); a batch with no
    valid pixel gives loss 0 and zero gradients (:84-88)."""
    from densematchingbenchmark_amd.modeling.stereo.losses import StereoFocalLoss
    gen = torch.Generator().manual_seed(521)
    gt = torch.rand((1, 1, 16, 24), generator=gen) * 30.0 + 1.0
    costs = [(rand((1, 32, 16, 24), 522)).requires_grad_(True), (rand((1, 16, 8, 12), 523)).requires_grad_(True)]
    want = [0.5 * O.stereo_focal_loss(costs[0], gt, 1.0, 32), 0.25 * O.stereo_focal_loss(
        costs[1], F_avg(gt / 2.0, (8, 12)), 1.0, 16)]
    got = StereoFocalLoss(max_disp=32, weights=(0.5, 0.25))([c.detach().to(dev).requires_grad_(True) for c in costs],
                                                            gt.to(dev), 1.0)
    for i in range(2):
        assert abs(float(got["stereo_focal_loss_lvl%d" % i].detach()) - float(want[i].detach())) <= 2e-5 * abs(float(want[i].detach()))
    c = torch.zeros((1, 8, 4, 4), device=dev, requires_grad=True)
    l = StereoFocalLoss(max_disp=8)(c, torch.full((1, 1, 4, 4), -1.0, device=dev), 1.0)["stereo_focal_loss_lvl0"]
    l.backward()
    assert float(l.detach()) == 0.0 and float(c.grad.abs().max()) == 0.0


def F_avg(x, hw):
    return torch.nn.functional.adaptive_avg_pool2d(x, hw)


def test_combined_loss_evaluator_vs_oracle(dev):
    """make_gsm_loss_evaluator(cfg) with the reference's AcfNet loss block: weighted dict of per-level terms."""
    from densematchingbenchmark_amd.config import Config
    from densematchingbenchmark_amd.modeling.stereo.losses import make_gsm_loss_evaluator
    cfg = Config(dict(data=dict(sparse=False), model=dict(losses=dict(
        focal_loss=dict(max_disp=32, start_disp=0, dilation=1, weight=1.0, weights=(1.0, 0.7), coefficient=5.0),
        l1_loss=dict(max_disp=32, weights=(0.1, 0.05), weight=2.0)))))
    ev = make_gsm_loss_evaluator(cfg)
    gen = torch.Generator().manual_seed(531)
    gt = torch.rand((1, 1, 12, 16), generator=gen) * 30.0 + 1.0
    costs = [rand((1, 32, 12, 16), 532), rand((1, 32, 12, 16), 533)]
    disps = [gt + rand((1, 1, 12, 16), 534), gt + rand((1, 1, 12, 16), 535) * 2]
    var = [0.5 + torch.rand((1, 1, 12, 16), generator=gen) for _ in range(2)]
    got = ev([d.to(dev) for d in disps], [c.to(dev) for c in costs], gt.to(dev), variance=[v.to(dev) for v in var])
    assert sorted(got) == ["l1_loss_lvl0", "l1_loss_lvl1", "stereo_focal_loss_lvl0", "stereo_focal_loss_lvl1"]
    for i, (wf, wl) in enumerate(((1.0, 0.1), (0.7, 0.05))):
        want_f = wf * 1.0 * float(O.stereo_focal_loss(costs[i], gt, var[i], 32, 0, 1, 5.0))
        want_l = wl * 2.0 * float(O.disp_smooth_l1_loss(disps[i], gt, 32))
        assert abs(float(got["stereo_focal_loss_lvl%d" % i]) - want_f) <= 2e-5 * abs(want_f)
        assert abs(float(got["l1_loss_lvl%d" % i]) - want_l) <= 2e-6


@pytest.mark.usefixtures("single_chain")
def test_backbone_views_on_two_streams_equal_one_batch(dev):
    """ops.two_view_forward: the two views of a pair through the PSMNet / GC-Net backbones as two chains on two HIP streams (the
    default: the partial tile rounds of one chain are filled by the other's) against one batch of both views -- the same launches
    per image, so bit-identical (on the single-chain kernels: under the default policy a view's smallest launches may take the
    split-K form where the batch of both views does not); and the caller's stream is joined (the features are usable right away)."""
    from densematchingbenchmark_amd import ops, synthetic
    from densematchingbenchmark_amd.modeling.stereo.backbones import PSMNetBackbone
    from densematchingbenchmark_amd.modeling.stereo.backbones.GCNet import GCNetBackbone
    for mk, shape in ((lambda: PSMNetBackbone(3, True), (2, 3, 256, 512)), (lambda: GCNetBackbone(3, True), (1, 3, 64, 128))):
        bb = mk().eval()
        synthetic.init_params_(bb, seed=8, classif_gain=1.0)
        bb = bb.to(dev)
        l, r = rand(shape, 441).to(dev), rand(shape, 442).to(dev)
        assert ops.view_streams()
        with torch.no_grad():
            fl, fr = bb(l, r)
            s = (fl.sum() + fr.sum()).item()             # consumed on the caller's stream without any explicit synchronisation
            ops.set_view_streams(False)
            try:
                gl, gr = bb(l, r)
            finally:
                ops.set_view_streams(True)
        assert torch.equal(fl, gl) and torch.equal(fr, gr) and s == (gl.sum() + gr.sum()).item()


def test_two_view_warm_up_sees_a_replaced_parameter(dev, monkeypatch):
    """ops.two_view_forward fills the packed-weight caches on the CALLER's stream before it forks the second view onto a side
    stream.  After a backbone Parameter object is replaced, that warm-up must run again -- otherwise the new packs are made
    inside one view's chain while the other view's chain reads them.  A spy on the replaced unit's ``_prepacked`` sees its first
    call on the caller's stream before the fork, and the features equal those of a freshly built backbone with the same weights."""
    import torch.nn as nn
    from densematchingbenchmark_amd import ops, synthetic
    from densematchingbenchmark_amd.modeling.stereo.backbones import PSMNetBackbone
    from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers_2d import FusedConv2d
    bb = PSMNetBackbone(3, True).eval()
    synthetic.init_params_(bb, seed=8, classif_gain=1.0)
    bb = bb.to(dev)
    l, r = rand((1, 3, 256, 512), 443).to(dev), rand((1, 3, 256, 512), 444).to(dev)
    assert ops.view_streams()
    with torch.no_grad():
        bb(l, r)                                             # warm: the caches hold the initial weights
    unit = [m for m in bb.modules() if isinstance(m, FusedConv2d)][-1]
    unit[0].weight = nn.Parameter(unit[0].weight.detach() * 0.5)
    events = []
    prepacked, side_stream = unit._prepacked, ops.side_stream

    def prepacked_spy():
        events.append(("prepacked", torch.cuda.current_stream(dev)))
        return prepacked()

    def side_stream_spy(*args):
        events.append(("fork", None))
        return side_stream(*args)

    monkeypatch.setattr(ops, "side_stream", side_stream_spy)
    unit._prepacked = prepacked_spy
    main = torch.cuda.current_stream(dev)
    try:
        with torch.no_grad():
            fl, fr = bb(l, r)
    finally:
        del unit._prepacked
    assert events and events[0] == ("prepacked", main), events[:3]
    fresh = PSMNetBackbone(3, True).eval().to(dev)
    fresh.load_state_dict(bb.state_dict())
    with torch.no_grad():
        gl, gr = fresh(l, r)
    assert torch.equal(fl, gl) and torch.equal(fr, gr)

