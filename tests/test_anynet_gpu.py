"""AnyNet on the MI355X: csrc/preact_conv.hip's units against CPU FP64 (FP32 as the scale), the bit-exact pieces, the stages
teacher-forced on the reference's recorded tensors (tests/golden/anynet.npz), the whole forward at full size against the
functional restatement (tests/_anynet_ref.py), invariance, launches and serving.

Full-size contract (``test_full_size_against_restatement``): |hip - fp64| against |restatement fp32 - fp64| of the same
weights and images, per output map, in max, mean and the count of pixels above 1e-4; see there for the measured numbers."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from densematchingbenchmark_amd import ops
from densematchingbenchmark_amd.config import Config
from tests import _anynet_ref as R
from tests.test_anynet_host import golden_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    return Config.fromfile(os.path.join(ROOT, "configs", "AnyNet", "scene_flow.py"))


def _model(dev, sd=None):
    from densematchingbenchmark_amd.modeling import build_model
    m = build_model(_cfg())
    m.load_state_dict(sd if sd is not None else golden_state(), strict=True)
    return m.to(dev).eval().requires_grad_(False)


def _within_fp32_scale(hip, ref64, ref32, what, factor=2.0, floor=1e-6):
    e_hip = (hip.double().cpu() - ref64).abs().max().item()
    e_32 = (ref32.double() - ref64).abs().max().item()
    bound = factor * e_32 + floor * max(1.0, ref64.abs().max().item())
    assert e_hip <= bound, (what, e_hip, e_32)


# ----------------------------------------------------------------------------------------------------------- kernel units
UNIT_CASES = [
    # ndim, B, Ci, Co, D, H, W, stride, pool, bn, pre_relu, post, relu, residual, windows
    (2, 1, 3, 1, 1, 17, 33, 1, False, False, False, "none", False, False, False),
    (2, 2, 1, 1, 1, 16, 40, 2, False, True, True, "none", False, False, False),
    (2, 2, 1, 2, 1, 15, 31, 1, True, True, True, "none", False, False, False),
    (2, 1, 12, 4, 1, 9, 21, 1, False, True, True, "none", False, False, True),
    (2, 2, 6, 2, 1, 1, 37, 1, False, True, True, "none", False, False, True),
    (2, 1, 4, 8, 1, 23, 3, 1, True, True, True, "none", False, False, False),      # 1 column after pooling
    (2, 1, 3, 16, 1, 12, 20, 1, False, False, False, "bn", True, False, False),
    (2, 1, 8, 1, 1, 13, 19, 1, False, False, False, "none", False, True, False),
    (2, 1, 2, 2, 1, 10, 10, 2, False, False, True, "bias", False, False, False),     # batch_norm=False: ReLU, Conv
    (2, 1, 64, 32, 1, 7, 9, 1, False, True, True, "bias", True, False, False),
    (3, 1, 8, 16, 12, 5, 9, 1, False, True, True, "bias", False, False, False),
    (3, 2, 16, 16, 5, 6, 35, 1, False, True, True, "bias", False, False, False),
    (3, 1, 4, 1, 5, 1, 7, 1, False, True, True, "bias", False, False, False),
    (3, 2, 2, 4, 5, 9, 1, 1, False, False, True, "bias", False, False, False),
]


def _unit_ref(x, w, stride, pool, ps, pt, pre_relu, post, sc, sh, relu, res):
    if pool:
        x = F.max_pool2d(x, 2, 2)
    if ps is not None:
        x = x * ps.view(1, -1, *([1] * (x.dim() - 2))) + pt.view(1, -1, *([1] * (x.dim() - 2)))
    if pre_relu:
        x = F.relu(x)
    y = (F.conv3d if x.dim() == 5 else F.conv2d)(x, w, None, stride, 1)
    shp = (1, -1) + (1,) * (y.dim() - 2)
    if post == "bn":
        y = y * sc.view(shp) + sh.view(shp)
    elif post == "bias":
        y = y + sh.view(shp)
    if relu:
        y = F.relu(y)
    if res is not None:
        y = F.relu(y + res)
    return y


@pytest.mark.parametrize("case", UNIT_CASES, ids=[str(i) for i in range(len(UNIT_CASES))])
def test_preact_conv_units(dev, case):
    ndim, B, Ci, Co, D, H, W, stride, pool, bn, pre_relu, post, relu, use_res, windows = case
    g = torch.Generator().manual_seed(1000 + UNIT_CASES.index(case))
    sp = (D, H, W) if ndim == 3 else (H, W)
    off, Ctot = (2, Ci + 5) if windows else (0, Ci)
    xfull = torch.randn((B, Ctot) + sp, generator=g)
    x = xfull[:, off:off + Ci]
    w = torch.randn((Co, Ci) + (3,) * ndim, generator=g) / (Ci * 3 ** ndim) ** 0.5
    ps = (torch.rand(Ci, generator=g) * 3 - 1.5) if bn else None           # gammas of both signs ...
    pt = (torch.randn(Ci, generator=g) + 2.0) if bn else None              # ... and betas with relu(beta) != 0: padding must stay 0
    sc = torch.rand(Co, generator=g) + 0.5
    sh = torch.randn(Co, generator=g)
    Hc, Wc = (H // 2, W // 2) if pool else (H, W)
    osp = ((D,) if ndim == 3 else ()) + ((Hc - 1) // stride + 1, (Wc - 1) // stride + 1)
    res = torch.randn((B, Co) + osp, generator=g) if use_res else None
    args = lambda t, dt: [None if a is None else a.to(dt) for a in t]         # noqa: E731
    refs = [_unit_ref(*args([x, w], dt), stride, pool, *args([ps, pt], dt), pre_relu, post, *args([sc, sh], dt), relu,
                      *args([res], dt)) for dt in (torch.float64, torch.float32)]
    d = lambda t: None if t is None else t.to(dev).contiguous()              # noqa: E731
    out, ooff = None, 0
    if windows:
        out, ooff = torch.full((B, Co + 3) + osp, 7.0, device=dev), 1
    y = ops.preact_conv(d(xfull), d(w), stride, pool, d(ps), d(pt), pre_relu, d(sc) if post == "bn" else None,
                        d(sh) if post != "none" else None, relu, d(res), False, (off, Ci), None, out, ooff)
    if windows:
        assert (y[:, :1] == 7.0).all() and (y[:, 1 + Co:] == 7.0).all()      # nothing outside the window is written
        y = y[:, 1:1 + Co]
    assert tuple(y.shape) == tuple(refs[0].shape)
    _within_fp32_scale(y, refs[0], refs[1], case)


def _resampled_close(got, want):
    """Half-pixel bilinear resampling in conv2d.hip's bilinear_hp arithmetic (as dmb_bilinear_scale_f32 and its test in
    test_kernels_gpu.py): torch's CPU kernel rounds its source index and weights differently in the last bits (measured: up to
    2 ulps of the taps, 1.9e-6 on maps of magnitude 15), so the bound is 1e-6 of the map's magnitude."""
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item()), (got - want).abs().max().item()


def test_exact_and_resampling_pieces(dev):
    """Max-pool (pool-then-scale, negative gammas) and gate normalisation given the same conv output: bit-exact against torch.
    The stage samples and the final maps: the same FP32 adds / differences as the reference, bit for bit, on resampled maps that
    agree with torch's to the last bits."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 19, 27, generator=g).to(dev)
    w = torch.randn(8, 4, 3, 3, generator=g).to(dev)
    ps, pt = (torch.rand(4, generator=g) * 3 - 1.5).to(dev), (torch.randn(4, generator=g) + 1).to(dev)
    fused = ops.preact_conv(x, w, 1, True, ps, pt, True)
    apart = ops.preact_conv(F.max_pool2d(x, 2, 2).contiguous(), w, 1, False, ps, pt, True)
    assert torch.equal(fused, apart)
    w24 = torch.randn(24, 16, 3, 3, generator=g).to(dev)
    f = torch.randn(1, 16, 11, 13, generator=g).to(dev)
    G = ops.preact_conv(f, w24)
    G1, G2, G3 = torch.split(G, 8, dim=1)
    s = G1.abs() + G2.abs() + G3.abs()
    for got, want in zip(ops.preact_conv(f, w24, gate=True), (torch.div(t, s + 1e-8) for t in (G1, G2, G3))):
        assert torch.equal(got, want)
    low = torch.randn(2, 1, 9, 17, generator=g) * 5
    lin = torch.linspace(-2, 2, 5)
    up, samples = ops.anynet_stage_samples(low.to(dev), (18, 34), 34 / 17, lin.to(dev))
    want = F.interpolate(low * (34 / 17), size=(18, 34), mode='bilinear', align_corners=False)
    _resampled_close(up.cpu(), want)
    assert torch.equal(samples.cpu(), lin.view(1, 5, 1, 1).expand(2, 5, 18, 34) + up.cpu())
    ds = [torch.randn(2, 1, h, w_, generator=g) * 3 for h, w_ in ((16, 32), (16, 32), (8, 16), (4, 8))]
    maps = ops.anynet_final_maps([t.to(dev) for t in ds], (64, 128))
    want = [F.interpolate(t * 128 / t.shape[-1], size=(64, 128), mode='bilinear', align_corners=False) for t in ds]
    for a, b in zip(maps, want):
        _resampled_close(a.cpu(), b)
    for i in range(1, 4):
        assert torch.equal(maps[3 + i], maps[i - 1] - maps[i])


# ----------------------------------------------------------------------------------------------------------- teacher-forced
def test_stages_teacher_forced(dev):
    """Each stage on the reference's recorded inputs (anynet.npz, batch 2 x 64x128), against the recorded FP64 forward with the
    recorded FP32 error as the scale.  Costs: fast_dif_fms multiplies by (warped > 0) (dif_fms.py:76-77), discontinuous where a
    warped target crosses 0: elements past the bound are COUNTED there; measured count: 0."""
    from tests.test_anynet_host import _golden
    z = _golden()
    m = _model(dev)
    t = lambda k: torch.from_numpy(z["f32/" + k]).to(dev)                    # noqa: E731
    r64 = lambda k: torch.from_numpy(z["f64/" + k])                          # noqa: E731
    r32 = lambda k: torch.from_numpy(z["f32/" + k])                          # noqa: E731
    left, right = (v.to(dev) for v in R.golden_inputs())
    with torch.no_grad():
        f16, f8, f4 = m.backbone.features(left, right)
        for s, f in ((16, f16), (8, f8), (4, f4)):
            _within_fp32_scale(f[:2], r64("fms_left_%d" % s), r32("fms_left_%d" % s), "fms_left_%d" % s)
            _within_fp32_scale(f[2:], r64("fms_right_%d" % s), r32("fms_right_%d" % s), "fms_right_%d" % s)
        proc, pred = m.cost_processor, m.disp_predictor
        costs = {"cost_init": proc.cost("init_guess", t("fms_left_16"), t("fms_right_16"), proc.samples("init_guess", dev))[0]}
        hw8, hw4 = tuple(t("fms_left_8").shape[-2:]), tuple(t("fms_left_4").shape[-2:])
        _, s8 = ops.anynet_stage_samples(t("disp_init"), hw8, 2.0, proc.samples("warp_level_8", dev))
        costs["cost_w8"] = proc.cost("warp_level_8", t("fms_left_8"), t("fms_right_8"), s8)[0]
        _, s4 = ops.anynet_stage_samples(t("disp_w8"), hw4, 2.0, proc.samples("warp_level_4", dev))
        costs["cost_w4"] = proc.cost("warp_level_4", t("fms_left_4"), t("fms_right_4"), s4)[0]
        flips = {}
        for k, c in costs.items():
            e = (c.double().cpu() - r64(k)).abs()
            bound = 2 * (r32(k).double() - r64(k)).abs().max().item() + 1e-6 * r64(k).abs().max().item()
            flips[k] = int((e > bound).sum())
        print("anynet teacher-forced cost elements past the bound:", flips)
        assert all(n <= 4 for n in flips.values()), flips
        for st, k, out in (("init_guess", "cost_init", "disp_init"), ("warp_level_8", "cost_w8", "res_w8"),
                           ("warp_level_4", "cost_w4", "res_w4")):
            _within_fp32_scale(pred[st](t(k)), r64(out), r32(out), out)
        up8, _ = ops.anynet_stage_samples(t("disp_init"), hw8, 2.0)
        _resampled_close(ops.add(up8, t("res_w8")).cpu(), r32("disp_w8"))       # combination
        up4, _ = ops.anynet_stage_samples(t("disp_w8"), hw4, 2.0)
        _resampled_close(ops.add(up4, t("res_w4")).cpu(), r32("disp_w4"))
        refined, _ = m.disp_refinement([t("disp_w4")], None, None, left, right)
        _within_fp32_scale(refined, r64("refined"), r32("refined"), "refined", factor=4.0)
        maps = ops.anynet_final_maps([t("refined"), t("disp_w4"), t("disp_w8"), t("disp_init")], (64, 128))
        _resampled_close(torch.stack(maps[:4]).cpu(), torch.from_numpy(z["f32/disps"]))


# ----------------------------------------------------------------------------------------------------------- end to end
def _fullsize_state():
    """The golden weights: seeded, BatchNorm with both signs of gamma."""
    return golden_state()


@pytest.mark.parametrize("B,H,W", [(1, 544, 960), (2, 544, 960), (1, 384, 1248)])
def test_full_size_against_restatement(dev, B, H, W):
    """The whole eval forward against tests/_anynet_ref.py on the CPU in FP64, with its FP32 evaluation as the scale, per map:
    max |hip - fp64| <= 4 * max |fp32 - fp64| + 1e-4, mean <= 4 * mean + 1e-6, count(> 1e-4) <= 2 * count + 0.001 * pixels.
    Measured on the 7 maps (golden weights, seeded images): max |hip - fp64| 2.2e-5 .. 3.4e-5 against 2.6e-5 .. 3.6e-5 for the
    FP32 restatement, means 3.4e-6 .. 4.7e-6 against 4.6e-6 .. 5.5e-6, and no pixel above 1e-4 on either side at 544x960
    (batch 1 and 2) and 384x1248: the HIP path is as close to FP64 as stock FP32 torch is.  The constants leave room for other
    weights without admitting a wrong tap or channel (those move maps by 1e-2 and more)."""
    sd = _fullsize_state()
    m = _model(dev, sd)
    left, right = R.golden_inputs((B, 3, H, W), 77 + B + H)
    cfg = _cfg().model.cost_processor
    with torch.no_grad():
        out, _ = m(dict(leftImage=left.to(dev), rightImage=right.to(dev)))
        r32, _ = R.forward(left, right, sd, cfg)
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        r64, _ = R.forward(left.double(), right.double(), sd64, cfg)
    stats = []
    for i, (h, a, b) in enumerate(zip(out["disps"], r32, r64)):
        eh, e32 = (h.double().cpu() - b).abs(), (a.double() - b).abs()
        n = eh.numel()
        stats.append((i, eh.max().item(), e32.max().item(), eh.mean().item(), e32.mean().item(), int((eh > 1e-4).sum()),
                      int((e32 > 1e-4).sum())))
    print("anynet full-size %dx%dx%d (map, max hip, max fp32, mean hip, mean fp32, >1e-4 hip, >1e-4 fp32):" % (B, H, W), stats)
    for i, mh, m32, ah, a32, ch, c32 in stats:
        assert mh <= 4 * m32 + 1e-4 and ah <= 4 * a32 + 1e-6 and ch <= 2 * c32 + 0.001 * n, stats[i]


# ----------------------------------------------------------------------------------------------------------- invariance
def test_batch_run_and_graph_invariance(dev):
    from densematchingbenchmark_amd.graph_runner import GraphedForward
    m = _model(dev)
    left, right = (t.to(dev) for t in R.golden_inputs((4, 3, 128, 256), 9))
    with torch.no_grad():
        full, _ = m(dict(leftImage=left, rightImage=right))
        again, _ = m(dict(leftImage=left, rightImage=right))
        for a, b in zip(full["disps"] + full["costs"], again["disps"] + again["costs"]):
            assert torch.equal(a, b)
        for i in range(4):
            one, _ = m(dict(leftImage=left[i:i + 1].contiguous(), rightImage=right[i:i + 1].contiguous()))
            for a, b in zip(full["disps"] + full["costs"], one["disps"] + one["costs"]):
                assert torch.equal(a[i:i + 1], b)
        one, _ = m(dict(leftImage=left[:1].contiguous(), rightImage=right[:1].contiguous()))
    runner = GraphedForward(m)
    batch = dict(leftImage=left[:1].contiguous(), rightImage=right[:1].contiguous())
    for _ in range(2):
        rep = runner(batch)[0]
        torch.cuda.synchronize()
        for a, b in zip(one["disps"] + one["costs"], rep["disps"] + rep["costs"]):
            assert torch.equal(a, b)


def test_launches_per_forward(dev):
    """One eval forward at batch 1: 14 (backbone) + 8 + 10 + 10 (stages) + 8 (refinement) + 1 (final maps) = 51 launches, all of
    them this library's; no MIOpen or ATen compute kernel."""
    from torch.profiler import ProfilerActivity, profile
    m = _model(dev)
    left, right = (t.to(dev) for t in R.golden_inputs((1, 3, 544, 960), 3))
    with torch.no_grad():
        m(dict(leftImage=left, rightImage=right))
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            m(dict(leftImage=left, rightImage=right))
            torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]
    print("anynet launches per forward:", len(kernels))
    assert len(kernels) <= 56, kernels
    assert len(kernels) == 51, kernels
    assert not [n for n in kernels if "miopen" in n.lower() or "at::native" in n or "MIOpen" in n], kernels


def test_serving(dev, tmp_path):
    """init_model(configs/AnyNet/scene_flow.py) -> inference_stereo on a synthetic PNG pair -> result.pkl in the reference
    layout."""
    from PIL import Image
    from densematchingbenchmark_amd import result_io
    from densematchingbenchmark_amd.apis import inference_stereo, init_model
    g = np.random.default_rng(4)
    img = (g.random((540, 960, 3)) * 255).astype(np.uint8)
    paths = {}
    for k, arr in (("left", img), ("right", np.roll(img, -4, axis=1))):
        p = tmp_path / ("%s.png" % k)
        Image.fromarray(arr).save(p)
        paths["%s_image_path" % k] = str(p)
    model = init_model(os.path.join(ROOT, "configs", "AnyNet", "scene_flow.py"), None, dev)
    model.load_state_dict({k: v.to(dev) for k, v in golden_state().items()}, strict=True)
    logged = inference_stereo(model, [paths], str(tmp_path / "log"), pad_to_shape=(544, 960))
    assert len(logged) == 1
    saved = result_io.load_result(os.path.join(str(tmp_path / "log"), "left", "result.pkl"))
    assert set(saved) == {"Result", "OriginalData"} and set(saved["Result"]) == {"disps", "costs"}
    assert len(saved["Result"]["disps"]) == 7 and len(saved["Result"]["costs"]) == 3
    assert all(tuple(d.shape[-2:]) == (540, 960) for d in saved["Result"]["disps"])
