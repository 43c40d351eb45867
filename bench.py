#!/usr/bin/env python
"""Headline benchmark: stereo pairs/s through the HIP cost-volume -> aggregation -> regression path.

    python bench.py --gpus N --steps K --warmup W          (N > 1: launched by torch.distributed.run, one rank/GPU)

Workload (BASELINE.json configs[1]): PSMNet cat-volume + stacked 3-D hourglass + 3x (trilinear up-sampling,
soft-argmin), 540x960 padded to 544x960, max_disp=192, batch 4 per GPU, FP32.  One "step" = one batch of 4
synthetic pairs through volume -> aggregator -> 3 disparity maps -> EPE accumulation; inputs (backbone feature
maps [4, 32, 136, 240] x 2) are resident in HBM before the timed region.  Pairs are sharded over ranks the way
the reference shards them (pair i -> rank i mod world, tools/test.py:108); the only collective is ONE SUM
all-reduce of the FP64 EPE accumulator over RCCL at the end of the job (inside the timed region).

Prints ONE JSON line (rank 0): ``value`` pairs/s and ``ms_per_step`` over the ``--steps`` timed steps.  A plain run does only
that: set up, ``--warmup`` untimed steps, the timed steps, ``--dump-outputs``, the line.

``--dump-outputs DIR`` writes what the last timed step computed -- the arrays a caller of the path receives (``disp<i>``,
``cost<i>``, ``conf<i>`` in the order of the model's result lists, FP32) and the FP64 EPE accumulator of the timed steps
(``epe_accumulator``) -- as DIR/<name>.npy, 60 MiB at most: an array above its share is written as a fixed, seeded sample of its
flattened elements.  The inputs are seeded, so two builds given the same arguments can be compared output for output.

``--full`` adds everything else (secondary figures, each after the timed region): ``roofline`` for the dominant kernel (conv3d
k3 s1 32->32, FP32 MFMA bound): algorithmic FLOP per launch / mean launch duration measured live with HIP events on the launch
stream inside the timed region; ``cpu_baseline`` times the CPU oracle (a port of the reference's PyTorch-CPU path) on the host:
1 warm-up + 3 timed full-size pairs, with the parity of pair 0 against it; the batch-1 latency legs,
the backbone end to end, the opt-in modes and the training step.  ``--no-cpu-baseline``, ``--no-extras``, ``--latency`` and
``--no-latency`` select among them.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from densematchingbenchmark_amd import ops, synthetic  # noqa: E402
from densematchingbenchmark_amd.config import Config  # noqa: E402
from densematchingbenchmark_amd.evaluation import EpeAccumulator  # noqa: E402
from densematchingbenchmark_amd.modeling import build_model  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_HBM_GBS = 8000.0
PATH_GFLOP_PER_PAIR = 1015.84   # SURVEY.md 8-d, PSMNet 544x960 D=192: the REFERENCE's formulation of the path
# what the path here EXECUTES per pair: dres0[0] runs as 2-D maps (csrc/catconv.hip): its 173.27 GFLOP become 6.5
PATH_GFLOP_PER_PAIR_EXECUTED = 1015.84 - 173.27 + 6.5
PATH_GB_PER_PAIR = 9.716        # module-boundary traffic per pair (each tensor read once + written once)
# the same three figures at the reference's published KITTI operating point, 384x1248 (932.18 GFLOP, 8.916 GB per pair;
# dres0[0] there is 2*27*64*32 * 48*96*312 = 159.01 GFLOP in the reference's formulation, 5.97 executed as 2-D maps)
PATH_FIGURES = {(544, 960, 192): (PATH_GFLOP_PER_PAIR, PATH_GFLOP_PER_PAIR_EXECUTED, PATH_GB_PER_PAIR),
                (384, 1248, 192): (932.18, 932.18 - 159.01 + 5.97, 8.916)}
PARITY_CONTRACT = "max|hip - fp64| <= max(1e-4, 1.25 * max|reference arithmetic - fp64|) and mean|hip - fp64| <= mean|reference arithmetic - fp64|"
DISTINCT_BATCHES = 4            # a rank cycles through this many distinct batches (16 distinct pairs at batch 4)
DOMINANT = "conv3d_k3_s1_32to32"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4, help="stereo pairs per GPU per step (cfg2: 4)")
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "PSMNet", "scene_flow.py"))
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs and the EPE accumulator as DIR/<name>.npy (60 MiB at most)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything besides the headline: roofline, CPU baseline + parity, latency, "
                         "backbone, opt-in modes, training step")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) no CPU baseline and parity check")
    ap.add_argument("--no-extras", action="store_true", help="(--full) skip the secondary legs (backbone, bf16x6, training step)")
    ap.add_argument("--conv3d-mode", default="exact", choices=["exact", "bf16x6"],
                    help="opt-in EXPERIMENT: 32-channel stride-1 layers on 3-way bf16 splits (FP32-equivalent accuracy, not "
                         "bit-identical); the headline is always measured with 'exact'")
    ap.add_argument("--latency", action="store_true", help="(--full) add the batch-1 latency legs (implied by --batch 1)")
    ap.add_argument("--no-latency", action="store_true", help="(--full) no latency legs even at --batch 1 (profiling runs)")
    ap.add_argument("--fused-regression", action="store_true",
                    help="opt-in fast path: fused up-sampling + soft-argmin, full-resolution costs not materialised")
    return ap.parse_args()


def _pick_threads():
    """The host has many more hardware threads than torch's CPU conv kernels can use well: time one full-size
    32->32 3x3x3 layer at a few thread counts (about a second each) and keep the fastest."""
    import torch.nn.functional as F
    ncpu = os.cpu_count() or 1
    cands = sorted({max(1, ncpu // k) for k in (1, 2, 4, 8)} | {min(ncpu, 16)}, reverse=True)
    x = torch.randn(1, 32, 48, 136, 240)
    w = torch.randn(32, 32, 3, 3, 3) * 0.03
    best, best_t = cands[0], float("inf")
    for n in cands:
        torch.set_num_threads(n)
        F.conv3d(x, w, padding=1)
        t0 = time.perf_counter()
        F.conv3d(x, w, padding=1)
        dt = time.perf_counter() - t0
        if dt < best_t:
            best, best_t = n, dt
    return best


def _fp64_truth(model, cfg, first_pair, ptype, agg, dev):
    """The exact value both FP32 evaluations approximate: the oracle's aggregator in FLOAT64 on the pair (evaluated by torch's
    own double kernels on the GPU: checker infrastructure, nothing of libdmb_hip.so), then an FP64 soft-argmin.  PSMNet / AcfNet
    concatenation configurations only; None otherwise."""
    from oracle import dmb_oracle as O   # checker only
    if ptype != "Concatenation" or agg not in ("PSMNet", "AcfNet"):
        return None
    md = cfg.model.max_disp
    left, right = first_pair
    try:
        with torch.no_grad():
            p64 = {k: (v.detach().double() if v.is_floating_point() else v.detach()).to(dev) for k, v in model.state_dict().items()}
            raw = O.cat_fms(left, right, md // 4, 0, 1).double().to(dev)
            fn = O.psm_aggregator if agg == "PSMNet" else O.acf_aggregator
            costs = fn(raw, p64, md, "cost_processor.aggregator.")
            out = [O.soft_argmin_f64(c.cpu(), md) for c in costs]
        del p64, raw, costs
        torch.cuda.empty_cache()
        return out
    except Exception as e:  # noqa: BLE001  (no double-precision convolution in this build, out of memory ...)
        print("bench.py: FP64 yardstick unavailable: %r" % (e,), file=sys.stderr)
        return None


def cpu_baseline(model, cfg, first_pair, ptype, agg, timed=3):
    """Oracle (port of the reference's CPU path) at the configuration's full size: 1 warm-up + ``timed`` timed evaluations of one
    pair (15-40 s of host time).  Returns the baseline record and the oracle's outputs for that pair
    (the parity check of this run)."""
    from oracle import dmb_oracle as O   # checker / reported baseline only -- never on the product path
    cores = _pick_threads()
    torch.set_num_threads(cores)
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    md = cfg.model.max_disp
    left, right = first_pair
    if ptype == "Correlation":
        run = lambda l, r: O.gwcnet_path(l, r, p, md, num_groups=cfg.model.cost_processor.cost_computation.get("num_groups", 40))  # noqa: E731
        what = "gwc + cat volume + PSMAggregator + 3x FasterSoftArgmin"
    elif agg == "AcfNet":
        if "cmn" in cfg.model:
            run = lambda l, r: O.acfnet_path(l, r, p, md, cmn_alpha=cfg.model.cmn.alpha, cmn_beta=cfg.model.cmn.beta)  # noqa: E731
            what = "cat_fms + AcfAggregator + 3x FasterSoftArgmin + Cmn"
        else:   # fixed-variance config: no confidence network
            def run(l, r):
                raw = O.cat_fms(l, r, md // 4, 0, 1)
                costs = O.acf_aggregator(raw, p, md, "cost_processor.aggregator.")
                return [O.faster_soft_argmin(c, md, 0, 1, 1.0, True) for c in costs], costs
            what = "cat_fms + AcfAggregator + 3x FasterSoftArgmin"
    elif agg == "StereoNet":
        run = lambda l, r: O.stereonet_path(l, r, p, md)  # noqa: E731
        what = "dif_fms + StereoNetAggregator + FasterSoftArgmin at 1/8 resolution"
    elif agg == "PSMNet":
        run = lambda l, r: O.psmnet_path(l, r, p, md)  # noqa: E731
        what = "cat_fms + PSMAggregator + 3x FasterSoftArgmin"
    else:
        return None, None
    # 1 warm-up + 3 timed pairs at the configuration's full size (the SAME pair each time: the
    # arithmetic does not depend on the data), mean s/pair; plus one full-size 32 -> 32 layer on ONE thread for scaling context
    times = []
    with torch.no_grad():
        t0 = time.perf_counter()
        outs = run(left, right)                       # warm-up at full size (thread pool, allocator, mkldnn primitives)
        cold = time.perf_counter() - t0
        for _ in range(timed):
            t0 = time.perf_counter()
            outs = run(left, right)
            times.append(time.perf_counter() - t0)
    shape = left[0].shape if isinstance(left, tuple) else left.shape
    tail = "features %dx%d, max_disp=%d (%s), torch CPU FP32, %d threads (fastest of a sweep on a %d-thread host)" % (
        shape[2], shape[3], md, what, cores, os.cpu_count() or 1)
    if not times:   # abbreviated (N > 1 jobs): the one cold pair
        return dict(value=1.0 / cold, unit="pairs/s", cores=cores, kind="port",
                    sample="1 pair without warm-up (%.2f s; abbreviated in multi-rank jobs, the N = 1 line carries BASELINE.md's "
                           "protocol), %s" % (cold, tail)), outs
    dt = sum(times) / len(times)
    return dict(value=1.0 / dt, unit="pairs/s", cores=cores, kind="port",
                sample="1 warm-up + %d timed pairs (mean %.2f s; each %s), %s" % (len(times), dt, [round(t, 2) for t in times], tail),
                single_thread_context=_single_thread_layer(cores)), outs


CPU_TIMED_PAIRS = 3


def _single_thread_layer(cores):
    """Scaling context: ONE full-size 32 -> 32 3x3x3 layer (86.6 GFLOP, 1/12 of a pair's arithmetic) on
    one thread and on the chosen thread count."""
    import torch.nn.functional as F
    x = torch.randn(1, 32, 48, 136, 240)
    w = torch.randn(32, 32, 3, 3, 3) * 0.03
    out = {}
    for n in (1, cores):
        torch.set_num_threads(n)
        F.conv3d(x[:, :, :8], w, padding=1)
        t0 = time.perf_counter()
        F.conv3d(x, w, padding=1)
        out["conv3d_32to32_fullsize_s_%dthr" % n] = round(time.perf_counter() - t0, 3)
    torch.set_num_threads(cores)
    return out


def _full_model(cfg, model, dev, seed=8):
    """``build_model(cfg)`` as the reference means it (backbone included), carrying the path model's weights; the backbone gets
    seeded ones.  None for configurations whose file names no backbone."""
    full = build_model(cfg).eval()
    if full.backbone is None:
        return None
    synthetic.init_params_(full.backbone, seed=seed, classif_gain=1.0)
    full.load_state_dict(model.state_dict(), strict=False)
    return full.to(dev)


def _image_inputs(first, world, B, H0, W0, Hp, Wp, dev, mean, std):
    """Synthetic image pairs as decoder bytes [B, H0, W0, 3], padded + normalised on the device the way the
    reference's transforms do it (StereoPad -> Normalize, csrc/preprocess.hip): [B, 3, Hp, Wp] x 2, resident in HBM."""
    lu8, ru8 = synthetic.image_batch(first, world, B, H0, W0, dev)
    return ops.stereo_pad_normalize(lu8, (Hp, Wp), mean, std), ops.stereo_pad_normalize(ru8, (Hp, Wp), mean, std)


def _timed(fn, steps, sync_each=False):
    """``steps`` evaluations between two synchronisations (back to back: the launch queues stay full), or -- ``sync_each`` -- each
    one followed by a synchronisation (what one caller of a serving API waits for)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
        if sync_each:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def end_to_end(cfg, model, dev, B, H0, W0, Hp, Wp, steps, check=True):
    """Secondary figure (not the headline metric): images -> PSMNet backbone (HIP conv2d) -> the path, on SYNTHETIC
    IMAGE pairs (textured left view, right view = left warped by the ground-truth field) that went through the data-side kernel;
    ``max_abs_disp``: pair 0 against the oracle's whole model (backbone + path) on the host."""
    full = _full_model(cfg, model, dev)
    if full is None:
        return None
    mean, std = cfg.data.eval.get("mean", ops.IMAGENET_MEAN), cfg.data.eval.get("std", ops.IMAGENET_STD)
    li, ri = _image_inputs(0, 1, B, H0, W0, Hp, Wp, dev, mean, std)
    batch = dict(leftImage=li, rightImage=ri)
    with torch.no_grad():
        res, _ = full(batch)                              # first pass packs the weights
        t_bb = _timed(lambda: full.backbone(li, ri), steps)
        t_all = _timed(lambda: full(batch), steps)
    out = {"pairs_per_s": round(B * 1e3 / t_all, 2), "ms_per_step": round(t_all, 3), "backbone_ms": round(t_bb, 3), "steps": steps,
           "note": "synthetic left/right IMAGES (uint8 [%d,%d,%d,3]) padded + normalised on the device (StereoPad -> Normalize, one launch per "
                   "view) to [%d,3,%d,%d], resident in HBM; build_model(cfg) with the HIP backbone (two views on two streams); %d "
                   "back-to-back steps between two synchronisations" % (B, H0, W0, B, Hp, Wp, steps)}
    if check and cfg.model.cost_processor.cost_aggregator.type == "PSMNet" and cfg.model.cost_processor.type == "Concatenation":
        from oracle import dmb_oracle as O   # checker only
        p = {k: v.detach().cpu() for k, v in full.state_dict().items()}
        with torch.no_grad():
            ref, _ = O.psmnet_model(li[0:1].cpu(), ri[0:1].cpu(), p, cfg.model.max_disp)
        out["max_abs_disp"] = [round((a[0:1].cpu() - b).abs().max().item(), 7) for a, b in zip(res["disps"], ref)]
        out["mean_abs_disp"] = [round((a[0:1].cpu() - b).abs().mean().item(), 8) for a, b in zip(res["disps"], ref)]
    del full
    torch.cuda.empty_cache()
    return out


def _reference_self_spread(ptype, agg_type, Hp, Wp, md):
    """max_ij |ref_i - ref_j| per level of the tracked self-spread fixture for THIS workload (PSMNet at 544x960 or 384x1248,
    max_disp 192), or None."""
    if ptype != "Concatenation" or agg_type != "PSMNet" or md != 192:
        return None
    tag = {(544, 960): "s544", (384, 1248): "kitti"}.get((Hp, Wp))
    path = os.path.join(ROOT, "tests", "golden", "fullsize_psmnet_spread.npz")
    if tag is None or not os.path.exists(path):
        return None
    import numpy as np
    g = np.load(path)
    return [float(g["%s_spread_full_disp%d" % (tag, k)]) for k in (3, 2, 1)]


def latency_leg(cfg, model, dev, first_batch, H0, W0, Hp, Wp, steps):
    """The batch-1 regime the reference publishes and serves in (configs/PSMNet/ResultOfPSMNet.md:15-19: 384x1248, B = 1;
    dmb/apis/inference.py:191-225: one pair per call): ONE pair through (a) the path alone (features -> disparities) and (b)
    build_model(cfg) whole (padded, normalised images -> disparities), each eagerly and replayed from a HIP graph
    (graph_runner.GraphedForward, the serving API's default at this size) -- as milliseconds one caller waits per pair (every
    call followed by a synchronisation) and as back-to-back pairs/s."""
    from densematchingbenchmark_amd.graph_runner import GraphedForward
    feats = {k: (tuple(t[0:1].contiguous() for t in v) if isinstance(v, tuple) else v[0:1].contiguous()) for k, v in first_batch.items()}
    n = max(5, steps)
    out = {"batch": 1, "calls_timed": n}
    ops.set_branch_overlap("auto")     # the library's default, as a caller of the serving API gets it

    def legs(fn_eager, batch, tag):
        with torch.no_grad():
            for _ in range(2):
                fn_eager(batch)
            e_sync, e_b2b = _timed(lambda: fn_eager(batch), n, True), _timed(lambda: fn_eager(batch), n)
        out[tag] = {"eager_ms_per_pair": round(e_sync, 3), "eager_back_to_back_ms": round(e_b2b, 3)}
        try:
            graphed = GraphedForward(fn_eager)
            for _ in range(2):
                graphed(batch)
            g_sync, g_b2b = _timed(lambda: graphed(batch), n, True), _timed(lambda: graphed(batch), n)
            with torch.no_grad():
                same = all(torch.equal(a, b) for a, b in zip(graphed(batch)[0]["disps"], fn_eager(batch)[0]["disps"]))
            out[tag].update({"graph_ms_per_pair": round(g_sync, 3), "graph_back_to_back_ms": round(g_b2b, 3),
                             "pairs_per_s_best": round(1e3 / min(e_b2b, g_b2b), 2), "graph_identical_to_eager": bool(same)})
            graphed.reset()
        except Exception as e:  # noqa: BLE001  (a capture failure must not lose the eager figures)
            out[tag]["graph_error"] = repr(e)[:300]

    legs(model, feats, "path")
    full = _full_model(cfg, model, dev)
    if full is not None:
        mean, std = cfg.data.eval.get("mean", ops.IMAGENET_MEAN), cfg.data.eval.get("std", ops.IMAGENET_STD)
        li, ri = _image_inputs(0, 1, 1, H0, W0, Hp, Wp, dev, mean, std)
        legs(full, dict(leftImage=li, rightImage=ri), "images_to_disparity")
        del full
    torch.cuda.empty_cache()
    ops.set_branch_overlap(False)
    out["note"] = ("library defaults (classifier branches on a second stream for one small pair); "
                   "ms_per_pair = mean wall time of one call followed by a synchronisation (inputs resident in HBM); graph = the "
                   "eval-mode forward captured once in a HIP graph and replayed (identical outputs); images_to_disparity = "
                   "build_model(cfg) with the HIP backbone on padded, normalised synthetic images")
    return out


def split_mode_leg(step, exact_disps, B, steps):
    """Secondary figure, NOT the headline: the same step with the stride-1 convolutions on exact 3-way bf16 splits of
    their FP32 operands (csrc/conv3d_x6.hip: FP32-equivalent accuracy, not bit-identical, never selected implicitly)."""
    ops.set_conv3d_mode("bf16x6")
    try:
        with torch.no_grad():
            for _ in range(2):
                disps = step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                disps = step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    finally:
        ops.set_conv3d_mode("exact")
    diff = [round((a - b).abs().max().item(), 7) for a, b in zip(disps, exact_disps)]
    return {"pairs_per_s": round(B * steps / dt, 2), "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps,
            "max_abs_disp_vs_exact_mode": diff,
            "note": "6 bf16 MFMA products per FP32 product, FP32 accumulate; see DESIGN.md section 8-1"}


def overlap_leg(step, exact_disps, B, steps):
    """Secondary figure, NOT the headline: the same step with the classifier branches on a second HIP stream next to the
    following hourglass (ops.set_branch_overlap): identical results, but concurrent kernels, so not the configuration the
    per-kernel roofline accounting is taken on."""
    ops.set_branch_overlap(True)
    try:
        with torch.no_grad():
            for _ in range(2):
                disps = step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                disps = step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    finally:
        ops.set_branch_overlap(False)
    same = all(torch.equal(a, b) for a, b in zip(disps, exact_disps))
    return {"pairs_per_s": round(B * steps / dt, 2), "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps,
            "identical_to_sequential": bool(same)}


def fused_leg(step_fused, exact_disps, B, steps):
    """Secondary figure, NOT the headline ("report both modes"): the same step with the up-sampling and the
    soft-argmin fused (dmb_trilinear_soft_argmin_f32) -- the three full-resolution cost volumes (3 x 1.6 GB at batch 4) are never
    written, so ``results['costs']`` does not exist in this mode; the disparity maps are the materialised mode's up to the
    regression's rounding."""
    with torch.no_grad():
        for _ in range(2):
            disps = step_fused()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            disps = step_fused()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    diff = [round((a - b).abs().max().item(), 7) for a, b in zip(disps, exact_disps)]
    return {"pairs_per_s": round(B * steps / dt, 2), "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps,
            "costs_materialised": False, "max_abs_disp_vs_materialised_mode": diff}


def training_leg(cfg, dev, steps):
    """Secondary figure, NOT the headline: one training iteration of the same cost path -- features -> volume ->
    aggregator with batch-statistics BatchNorm -> fused regression -> weighted smooth-L1, backward through the HIP kernels,
    Adam step -- at the reference's training shape (256 x 512 crops, configs/PSMNet/scene_flow.py), batch 4."""
    from densematchingbenchmark_amd.dist_utils import FlatGradients
    B, H, W = 4, 256, 512
    model = build_model(cfg, backbone=None).to(dev)
    synthetic.init_params_(model, seed=0)
    model.train()
    flat = FlatGradients(model)
    opt = torch.optim.Adam(flat.params, lr=1e-3, fused=True)   # (torch's one-launch Adam; rounds 1-5 timed its 11-launch multi-tensor form)
    g = torch.Generator().manual_seed(7)
    batch = dict(leftFeature=torch.randn((B, 32, H // 4, W // 4), generator=g).to(dev),
                 rightFeature=torch.randn((B, 32, H // 4, W // 4), generator=g).to(dev),
                 leftDisp=(torch.rand((B, 1, H, W), generator=g) * 180.0 + 1.0).to(dev))

    def one():
        flat.zero_()
        _, losses = model(batch)
        sum(losses.values()).backward()
        opt.step()

    for _ in range(2):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # arithmetic of one iteration in the REFERENCE's formulation = forward + data gradients + weight gradients = 3 x the forward's
    # (SURVEY 8-d figure scaled by the crop's area; the data gradient of the first layer is not needed when the features are
    # inputs, but the figure is kept as the yardstick of rounds 1-5).  EXECUTED since round 6: the first layer runs as 2-D maps
    # in the forward pass and in its weight gradient -- rocprofv3 counts 2624 GFLOP of matrix instructions per step
    # (profiles/r06_train_pmc.csv; 3048 in round 5)
    gflop = 3.0 * PATH_GFLOP_PER_PAIR * (H * W) / (544.0 * 960.0) * B
    gflop_exec = 2623.5 * B / 4.0
    out = {"pairs_per_s": round(B * steps / dt, 2), "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps,
           "workload": "PSMNet cost path, training mode, batch %d x %dx%d crops, max_disp=192, Adam" % (B, H, W),
           "gflop_per_step": round(gflop, 1), "frac_fp32_peak": round(gflop / (dt / steps) / 1e3 / PEAK_FP32_MFMA_TFLOPS, 4),
           "gflop_per_step_executed": gflop_exec,
           "frac_fp32_peak_executed": round(gflop_exec / (dt / steps) / 1e3 / PEAK_FP32_MFMA_TFLOPS, 4),
           "optimizer": "torch.optim.Adam(fused=True)", "per_kernel_roofline": "profiles/r06_train_pmc.csv",
           "peak_memory_gb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)}
    del model, flat, opt, batch
    torch.cuda.empty_cache()
    return out


def roofline(timer, B, d4, h4, w4, conv3d_mode):
    """(--full) The dominant kernel's launches as timed live in the timed region (``timer``) against the FP32 matrix peak."""
    kms = timer.mean_ms(DOMINANT)
    flop = 2.0 * 27 * 32 * 32 * B * d4 * h4 * w4
    achieved = flop / (kms * 1e-3) / 1e12
    # `traffic` is NOT measured by this run: it is the PMC figure (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same
    # command, scripts/profile.sh) of the tracked profile summary, valid for the workload that summary was taken on
    traffic, traffic_source = None, None
    import glob
    for pmc in sorted(glob.glob(os.path.join(ROOT, "profiles", "pmc_dominant*.json")), reverse=True):   # one summary per profiled workload
        try:
            rec = json.load(open(pmc))
            if tuple(rec.get("shape", [])) == (B, 32, d4, h4, w4):
                traffic = rec.get("hbm_bytes_per_launch")
                traffic_source = "profiles/%s (rocprofv3 PMC passes of an earlier run of this command: %s)" % (
                    os.path.basename(pmc), rec.get("derived_from", "see the file"))
                break
        except Exception:  # noqa: BLE001
            continue
    out = {"kernel": "conv3d_s1_kernel<32,32> (k3 s1 32->32, [%d,32,%d,%d,%d])" % (B, d4, h4, w4),
           "bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_FP32_MFMA_TFLOPS,
           "unit": "TFLOP/s", "frac": round(achieved / PEAK_FP32_MFMA_TFLOPS, 4), "traffic": traffic,
           "traffic_source": traffic_source,
           "launch_ms": round(kms, 4), "launches_timed": timer.count(DOMINANT),
           "timed_every_nth_step": timer.every,
           "flop_per_launch": flop}
    if conv3d_mode != "exact":   # the split kernel issues 6 bf16 MFMAs per FP32 product (+ 28/27 tap padding)
        issued = achieved * 6.0 * 28.0 / 27.0
        out.update({"kernel": "conv3d_s1_x6_kernel (k3 s1 32->32, bf16x6 split)", "achieved": round(issued, 1),
                    "peak": 2500.0, "frac": round(issued / 2500.0, 4),
                    "fp32_equivalent_tflops": round(achieved, 2), "traffic": None})
    return out


DUMP_BUDGET_BYTES = 60 * 2 ** 20


def dump_outputs(directory, arrays):
    """``arrays`` (name -> tensor) as ``directory``/<name>.npy: FP64 tensors as FP64, everything else as FP32, DUMP_BUDGET_BYTES in
    all.  Smallest first, each array gets an equal share of what is left; one that is larger is written as the elements at a
    fixed, seeded sample of its flattened indices (sorted: the same positions in every run and every build).  The sample is drawn
    by numpy on the host: torch.randperm of a few million elements took 15 s per call in a process that had run the path."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    host = {}
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        host[name] = a.astype(np.float64 if a.dtype == np.float64 else np.float32, copy=False)
    left, samples = DUMP_BUDGET_BYTES, {}
    for n, name in enumerate(sorted(host, key=lambda k: host[k].nbytes)):
        a = host[name]
        cap = left // (len(host) - n) // a.itemsize
        if a.size > cap:
            if (a.size, cap) not in samples:
                samples[(a.size, cap)] = np.sort(np.random.default_rng(0).choice(a.size, size=cap, replace=False))
            a = a.reshape(-1)[samples[(a.size, cap)]]
        np.save(os.path.join(directory, name + ".npy"), a)
        left -= a.nbytes


def pin_to_gpu_numa_node(local_rank):
    """Bind this rank's host threads to the CPUs of the NUMA node its GPU hangs off (the reference leaves placement to the OS;
    with eight ranks on a two-socket host a rank whose launch thread runs on the far socket pays a cross-socket hop per launch).
    Returns a description for the JSON line; silently does nothing where sysfs does not tell (containers without /sys/bus/pci)."""
    try:
        prop = torch.cuda.get_device_properties(local_rank)
        bdf = "%04x:%02x:%02x.0" % (getattr(prop, "pci_domain_id", 0), prop.pci_bus_id, prop.pci_device_id)
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % bdf).read().strip())
        if node < 0:
            return {"gpu_pci": bdf, "numa_node": node, "pinned": False}
        cpus = set()
        for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
        cpus &= os.sched_getaffinity(0)
        if not cpus:
            return {"gpu_pci": bdf, "numa_node": node, "pinned": False}
        os.sched_setaffinity(0, cpus)
        return {"gpu_pci": bdf, "numa_node": node, "pinned": True, "cpus": len(cpus)}
    except Exception as e:  # noqa: BLE001
        return {"pinned": False, "why": repr(e)[:80]}


def launch_ranks(n):
    """``python bench.py --gpus N`` started as ONE process: re-run this script as N ranks, one per GPU, under
    torch.distributed.run (the shape of the reference's tools/dist_test.sh:9-10 -> tools/test.py:101-208).  The driver's
    own ``python -m torch.distributed.run ... bench.py --gpus N`` arrives with WORLD_SIZE set and skips this."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n, "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    # DMB_BENCH_BACKEND=gloo is a test hook: several ranks may then share one GPU (RCCL refuses duplicate devices), which
    # exercises the whole multi-rank control flow of this script on a single-GPU box.
    backend = os.environ.get("DMB_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank %= torch.cuda.device_count()
    elif world > torch.cuda.device_count():
        raise SystemExit("bench.py: %d ranks but %d visible GPUs (one rank per GPU over RCCL)" % (world, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    all_cpus = os.sched_getaffinity(0)
    affinity = pin_to_gpu_numa_node(local_rank) if world > 1 else {"pinned": False, "why": "single rank"}
    # DMB_BENCH_FORCE_PG=1: a ONE-rank job also goes through the process group, so that RCCL initialisation, the FP64
    # accumulator all-reduce, the barrier fence and the MAX clock reduce -- the exchange of tools/test.py:172-208 -- execute on
    # whatever hardware is there (tests/test_bench_gpu.py runs it on the single leased MI355X)
    use_pg = world > 1 or os.environ.get("DMB_BENCH_FORCE_PG", "0") == "1"
    if use_pg:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if "MASTER_PORT" not in os.environ:
            sk = socket.socket()
            sk.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
            sk.close()
        kw = dict(device_id=dev) if backend == "nccl" else {}
        dist.init_process_group(backend=backend, rank=rank, world_size=world, **kw)  # nccl == RCCL on ROCm

    cfg = Config.fromfile(args.config)
    md = cfg.model.max_disp
    Hp, Wp = cfg.data.eval.input_shape
    H0, W0 = cfg.data.eval.get("original_shape", cfg.data.eval.input_shape)
    scale = md // cfg.model.cost_processor.cost_computation.max_disp
    fh, fw = Hp // scale, Wp // scale
    C = 32
    B = args.batch

    ops.set_conv3d_mode(args.conv3d_mode)
    # the timed loop and the per-kernel roofline figures are taken WITHOUT concurrent kernels: the classifier-branch overlap (on by
    # default for one small pair, ops.set_branch_overlap("auto")) is switched off here and left to the latency / overlap legs
    ops.set_branch_overlap(False)
    model = build_model(cfg, backbone=None).eval()
    synthetic.init_params_(model, seed=0, classif_gain=10.0)
    model = model.to(dev)
    n_ids = len(cfg.get("eval_disparity_id", [0]))

    # inputs resident in HBM before the timed region.  The job's pairs are numbered globally and pair i goes to rank i mod world
    # (tools/test.py:108); a rank holds DISTINCT_BATCHES distinct local batches (16 distinct pairs at batch 4) and step k
    # evaluates batch k mod DISTINCT_BATCHES, so the "dataset" metrics and the sharding rule run over many pairs, not over four
    ptype = cfg.model.cost_processor.type
    pred_scale = md // cfg.model.disp_predictor.max_disp   # StereoNet regresses at 1/8 resolution
    nb = max(1, min(DISTINCT_BATCHES, args.steps))
    batches = []
    for k in range(nb):
        first = rank + world * B * k     # this rank's pairs of batch k: first, first + world, ...
        if ptype == "Correlation":   # GwcNet-style: (320-ch correlation features, 12-ch concat features) per view
            lg, rg = synthetic.feature_batch(first, world, B, 320, fh, fw, dev)
            lc, rc = synthetic.feature_batch(first + 100000, world, B, 12, fh, fw, dev)
            lft, rgt = (lg, lc), (rg, rc)
        else:
            lft, rgt = synthetic.feature_batch(first, world, B, C, fh, fw, dev)
        g_k = synthetic.gt_batch(first, world, B, Hp // pred_scale, Wp // pred_scale, pad_top=(Hp - H0) // pred_scale, device=dev)
        if pred_scale > 1:
            g_k = g_k / pred_scale
        batches.append((dict(leftFeature=lft, rightFeature=rgt), g_k))
    left, right = batches[0][0]["leftFeature"], batches[0][0]["rightFeature"]
    acc = EpeAccumulator(dev, n_ids, cfg.model.eval.lower_bound, cfg.model.eval.upper_bound)
    fused = args.fused_regression
    counter = [0]

    last_results = {}

    def step(k=None, fused=fused, keep=False):
        """One step; ``keep``: hold on to everything the model returned (the last timed step, for --dump-outputs)."""
        if k is None:
            k = counter[0]
            counter[0] += 1
        batch, gt = batches[k % nb]
        left, right = batch["leftFeature"], batch["rightFeature"]
        if not fused:
            results, _ = model(batch)
            disps = results["disps"]
            last_results.clear()
            last_results.update({name: v for name, v in results.items() if keep or name == "confs"})
        else:
            agg = model.cost_processor.aggregator
            if ops.cat_fusion() and ptype == "Concatenation":   # the volume-free first layer, as the default mode runs it
                from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils.cat_fms import LazyCatVolume
                raw = LazyCatVolume(left, right, kind="cat", **model.cost_processor.default_args)
            else:
                raw = model.cost_processor.vol_func(left, right, **model.cost_processor.default_args)
            c1, c2, c3 = agg.trunk(raw)
            vals = model.disp_predictor._sample_values()
            disps = [ops.trilinear_soft_argmin(c.squeeze(1), (md, Hp, Wp), vals, model.disp_predictor.alpha)
                     for c in (c3, c2, c1)]
        acc.update(disps[:n_ids], gt, (H0 // pred_scale, W0 // pred_scale))
        return disps

    def fence():
        torch.cuda.synchronize()
        if use_pg:
            dist.barrier()
        torch.cuda.synchronize()

    with torch.no_grad():
        for _ in range(args.warmup):
            disps = step()
        acc.acc.zero_()
        counter[0] = 0
        # --full: live HIP-event timing of the dominant kernel's launches inside the timed region: every launch of every step for
        # short runs, of every (steps / 4)-th step from 16 steps on (>= 24 timed launches either way; each bracketed launch costs its
        # stream ~10 us) (round 6: every (steps / 4)-th step = 24 timed launches of a PSMNet step's six -- at one 256x512 pair the
        # 10 us per bracketed launch were 1.5 % of the step when every 4th step was timed).  A plain run brackets nothing.
        timer = ops.KernelTimer([DOMINANT], every=max(1, args.steps // 4) if args.steps >= 16 else 1) if args.full else None
        ops.set_kernel_timer(timer)
        dump = args.dump_outputs is not None and rank == 0
        fence()
        t0 = time.perf_counter()
        for i in range(args.steps):
            if timer is not None:
                timer.begin_step()
            disps = step(keep=dump and i == args.steps - 1)
        acc.all_reduce()
        fence()
        elapsed = time.perf_counter() - t0
        ops.set_kernel_timer(None)

    tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")   # (gloo gathers host tensors)
    per_rank_ms = [elapsed / args.steps * 1e3]
    if use_pg:
        gathered = [torch.zeros_like(tmax) for _ in range(world)]
        dist.all_gather(gathered, tmax)            # every rank's own clock, not only the MAX the metric is computed from
        per_rank_ms = [g.item() / args.steps * 1e3 for g in gathered]
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    elapsed = tmax.item()
    pairs = B * args.steps * world
    value = pairs / elapsed
    metrics = acc.summary()

    if dump:   # (rank 0) what the last timed step returned, and the accumulator of all timed steps
        arrays = {"disp%d" % i: d for i, d in enumerate(disps)}
        for key in ("costs", "confs"):
            arrays.update({"%s%d" % (key[:-1], i): t for i, t in enumerate(last_results.get(key) or []) if torch.is_tensor(t)})
        arrays["epe_accumulator"] = acc.acc
        dump_outputs(args.dump_outputs, arrays)
        del arrays
        last_results.pop("costs", None)

    if rank == 0:
        d4, h4, w4 = md // scale, fh, fw
        out = {
            "metric": "stereo pairs/s (%dx%d, max_disp=%d)" % (H0, W0, md), "value": round(value, 3), "unit": "pairs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "pairs": pairs,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32" if args.conv3d_mode == "exact" else "f32 as 3 bf16 pieces (6 products, f32 accumulate)",
            "data": "synthetic",
            "config": {"workload": "%s %s-volume + 3D aggregation + soft-argmin, %dx%d (%dx%d padded), "
                                   "max_disp=%d, batch %d per GPU%s" % (cfg.model.cost_processor.cost_aggregator.type, ptype, Hp, Wp, H0, W0, md, B,
                                                                        ", fused up-sample+regression" if fused else ""),
                       "pairs_per_step_per_gpu": B, "sharding": "pair i -> rank i mod world; 1 all-reduce of the EPE accumulator",
                       "costs_materialised": not fused, "conv3d_mode": args.conv3d_mode},
            "first_layer": ("3-D convolution on the materialised volume" if not ops.cat_fusion() else
                            {"Concatenation": "2-D maps, volume not materialised (csrc/catconv.hip)",
                             "Difference": "2-D maps, volume not materialised (csrc/catconv.hip)",
                             "Correlation": "correlation channels 3-D, concat channels as 2-D maps (csrc/catconv.hip)"}.get(ptype, "3-D convolution")),
            "epe_accumulator": metrics[0],
            "per_rank_ms": [round(t, 3) for t in per_rank_ms],
            "host_affinity": affinity,
        }
        if use_pg and backend == "nccl":
            try:
                out["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:  # noqa: BLE001
                out["rccl_version"] = None
        if ptype == "Concatenation" and cfg.model.cost_processor.cost_aggregator.type == "PSMNet" and (Hp, Wp, md) in PATH_FIGURES:
            gf_ref, gf_exec, gb = PATH_FIGURES[(Hp, Wp, md)]
            if not ops.cat_fusion():
                gf_exec = gf_ref
            # arithmetic of the REFERENCE's formulation per second (1015.84 GFLOP per pair at 544x960, 932.18 at
            # 384x1248); the path itself executes less (dres0[0] in its 2-D form: 2/3 of that layer's multiplications do not exist)
            out["path_gflop_per_pair"] = {"reference_formulation": gf_ref, "executed": round(gf_exec, 2)}
            out["path_tflops_reference_formulation"] = round(value * gf_ref / 1e3, 2)
            # NOT a roofline fraction: the reference's formulation counts 173 GFLOP per pair that the volume-free first layer never
            # executes -- this is the speed-up over executing that formulation at the matrix peak
            out["path_speed_vs_reference_formulation_at_fp32_peak"] = round(value * gf_ref / 1e3 / world / PEAK_FP32_MFMA_TFLOPS, 4)
            # ... and the arithmetic the path really EXECUTES: the achieved fraction of the matrix peak
            out["path_tflops_executed"] = round(value * gf_exec / 1e3, 2)
            out["path_frac_fp32_peak_executed"] = round(value * gf_exec / 1e3 / world / PEAK_FP32_MFMA_TFLOPS, 4)
            # north_star: throughput as a fraction of the HBM roofline (module-boundary traffic per pair / 8 TB/s;
            # the path is compute-bound, the FP32 matrix peak caps this fraction at 0.188)
            out["path_hbm_gbs_algorithmic"] = round(value * gb, 1)
            out["path_frac_hbm_roofline"] = round(value * gb / world / PEAK_HBM_GBS, 4)
        if args.full:
            out["roofline"] = roofline(timer, B, d4, h4, w4, args.conv3d_mode)
        agg_type = cfg.model.cost_processor.cost_aggregator.type
        out["distinct_pairs_per_gpu"] = nb * B
        if args.full:
            with torch.no_grad():
                disps = step(0)      # batch 0 again: the parity check and the secondary legs below all look at global pair 0
        if args.full and not args.no_cpu_baseline:
            first = tuple(t[0:1].cpu() for t in left) if isinstance(left, tuple) else left[0:1].cpu()
            first_r = tuple(t[0:1].cpu() for t in right) if isinstance(right, tuple) else right[0:1].cpu()
            # BASELINE.md's protocol (1 warm-up + 3 timed pairs) at every N: the other ranks have left the timed region and wait at
            # the final barrier below; this rank's host threads go back to the whole machine first (they were pinned to one node)
            os.sched_setaffinity(0, all_cpus)
            base, ref = cpu_baseline(model, cfg, (first, first_r), ptype, agg_type, timed=CPU_TIMED_PAIRS)
            if base is not None:
                out["cpu_baseline"] = base
                out["speedup_vs_cpu"] = round(value / base["value"], 1)
                # parity of global pair 0 against the oracle's outputs for that pair
                d_gpu = [d[0:1].cpu() for d in disps]
                out["parity_vs_cpu"] = {"max_abs_disp": [round((a - b).abs().max().item(), 7) for a, b in zip(d_gpu, ref[0])],
                                        "epe_delta": [round((a - b).abs().mean().item(), 8) for a, b in zip(d_gpu, ref[0])]}
                # north_star asks for 1e-4 max-abs against the reference's CPU path.  At max_disp = 192 the reference's own FP32
                # arithmetic sits 1.2 .. 2.5e-4 from the exact value, so the contract the tests enforce is a
                # RELAXATION of north_star, stated here with both distances from an FP64 evaluation of the same network:
                truth = _fp64_truth(model, cfg, (first, first_r), ptype, agg_type, dev)
                out["parity_vs_cpu"]["north_star_bound"] = 1e-4
                out["parity_vs_cpu"]["north_star_met"] = bool(max(out["parity_vs_cpu"]["max_abs_disp"]) <= 1e-4)
                spread = _reference_self_spread(ptype, agg_type, Hp, Wp, md)
                if spread is not None:     # how far the reference is from ITSELF on this workload (a tracked fixture, not measured here)
                    bound = max(1e-4, 1.6 * max(spread))
                    out["parity_vs_cpu"]["reference_self_spread"] = {
                        "max_abs_disp_between_1_3_8_host_threads": [round(v, 7) for v in spread],
                        "bound_on_hip_vs_reference": round(bound, 7), "rule": "max(1e-4, 1.6 x the largest self-spread)",
                        "within_bound": bool(max(out["parity_vs_cpu"]["max_abs_disp"]) <= bound),
                        "source": "tests/golden/fullsize_psmnet_spread.npz (oracle/gen_golden_fullsize.py spread: the REAL reference, pair 0, "
                                  "same weights and inputs, torch.set_num_threads(1 / 3 / 8); whole maps, levels 3 / 2 / 1)"}
                if truth is None:    # (only PSMNet / AcfNet concatenation configurations have an FP64 evaluation; or it failed: stderr)
                    out["parity_vs_cpu"]["fp64_yardstick"] = "unavailable"
                if truth is not None:
                    e_hip = [(a.double() - t).abs() for a, t in zip(d_gpu, truth)]
                    e_ref = [(b.double() - t).abs() for b, t in zip(ref[0], truth)]
                    out["parity_vs_cpu"].update({
                        "fp64_yardstick": "torch FP64 kernels on the GPU, oracle's aggregator",
                        "parity_contract": PARITY_CONTRACT,
                        "parity_contract_proof": "tests/test_oracle_golden.py::test_reference_faster_soft_argmin_is_an_fp32_fma_chain_bit_for_bit, "
                                                 "::test_reproducing_the_reference_order_cannot_meet_1e4_without_bit_identical_costs",
                        "max_abs_disp_vs_fp64": [round(e.max().item(), 7) for e in e_hip],
                        "reference_arithmetic_max_abs_disp_vs_fp64": [round(e.max().item(), 7) for e in e_ref],
                        "mean_abs_disp_vs_fp64": [round(e.mean().item(), 8) for e in e_hip],
                        "reference_arithmetic_mean_abs_disp_vs_fp64": [round(e.mean().item(), 8) for e in e_ref],
                        "contract_met": bool(all(h.max().item() <= max(1e-4, 1.25 * r.max().item()) and h.mean().item() <= r.mean().item()
                                                 for h, r in zip(e_hip, e_ref)))})
                if len(ref) > 2 and "confs" in last_results:
                    out["parity_vs_cpu"]["max_abs_conf"] = [round((a[0:1].cpu() - b).abs().max().item(), 7)
                                                            for a, b in zip(last_results["confs"], ref[2])]
        if args.full and world == 1 and (B == 1 or args.latency) and not args.no_latency and not fused and args.conv3d_mode == "exact":
            # the batch-1 / serving regime (dmb/apis/inference.py:191-225): ms per pair, eager and replayed from a HIP graph
            out["latency"] = latency_leg(cfg, model, dev, batches[0][0], H0, W0, Hp, Wp, min(args.steps, 20))
        if args.full and world == 1 and ptype == "Concatenation" and agg_type == "PSMNet" and not fused and not args.no_extras:
            out["end_to_end_with_backbone"] = end_to_end(cfg, model, dev, B, H0, W0, Hp, Wp, min(args.steps, 5), check=not args.no_cpu_baseline)
            if args.conv3d_mode == "exact":
                out["opt_in_branch_overlap"] = overlap_leg(lambda: step(0), disps, B, min(args.steps, 10))
                out["opt_in_fused_regression"] = fused_leg(lambda: step(0, fused=True), disps, B, min(args.steps, 10))
                out["opt_in_bf16x6"] = split_mode_leg(lambda: step(0), disps, B, min(args.steps, 5))
                if "losses" in cfg.model:
                    out["training_step"] = training_leg(cfg, dev, min(args.steps, 5))
        print(json.dumps(out), flush=True)
    if use_pg:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
