"""DeepPruner's refinement under autograd on one GPU, by the method of docs/design/17: each figure is the median of ``--repeats``
HIP-event timings of ``--iters`` back-to-back calls after a warm-up, with spread = max - min of those timings.

(a) ``--only wgrad``: the weight gradient of the head's classifier, ``ops.conv2d_wgrad(x, dc, 3, 1)`` with one output channel, at
    x [1 | 4, 16, 128, 256] and [1 | 4, 16, 272, 480], against ``torch.nn.grad.conv2d_weight``.  Each line names the plan code the
    loaded library reports: 0x700 (form 7) here.  Run on a build of the PARENT commit (a tagged development build: DMB_LIB=dev_<tag>,
    densematchingbenchmark_amd/build.py) the same lines measure the parent's launch of the same description, plan 0x400; such a
    build is bound through ctypes, so ``DMB_SHIM=0`` gives this commit's figures through the same binding.
(b) ``--only stages``: ``train_fn.deeppruner_refinement`` forward + backward against stock PyTorch-ROCm autograd through the
    restatement (tests/_deeppruner_features_ref.py) with the same weights on the SAME GPU, modules in train(): the 4x config's one
    stage (guide [B, 42, 128, 256]: 41 feature channels and the disparity) and the 8x config's two (guides [B, 74, 64, 128] and
    [B, 33, 128, 256]) for a 256 x 512 training crop, batch 1 and 4.  Each line also holds the host's issue time per pass.
(c) ``--only tail``: ``train_fn.refinement_head`` forward + backward alone at the stages' sizes, its share of the stage, and the two
    candidates for its data gradient (``ops.preact_conv`` on the mirrored weight against ``ops.conv2d_dgrad``).

Exits non-zero unless the HIP path is faster than stock at every measured stage and batch.

    python scripts/bench_deeppruner_refinement_bwd.py [--iters 10] [--repeats 5] [--out profiles/deeppruner_refinement_bwd_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from densematchingbenchmark_amd import _lib, ops  # noqa: E402

WGRAD_SIZES = [(1, 16, 128, 256), (4, 16, 128, 256), (1, 16, 272, 480), (4, 16, 272, 480)]
# config -> (in_planes_list, (H, W) of the first stage) at a 256 x 512 crop
CONFIGS = {"4x": ([32 + 9 + 1], (128, 256)), "8x": ([64 + 9 + 1, 32 + 1], (64, 128))}


def timed(fn, iters, repeats, warmup=3):
    """(median, max - min, median issue time) of ``repeats`` timings of ``iters`` back-to-back calls, ms per call.  The issue time
    is what the host needs to hand the calls to the stream (wall clock, before the synchronisation): where it equals the event
    time the host, not the GPU, bounds the figure."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms, issue = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        issue.append((time.perf_counter() - t0) * 1e3 / iters)
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return statistics.median(ms), max(ms) - min(ms), statistics.median(issue)


def _put(res, key, timing):
    res[key + "_ms"], res[key + "_spread_ms"], res[key + "_issue_ms"] = timing


def wgrads(args, dev):
    lines = []
    binding = "ctypes" if _lib.shim() is None else "shim"
    for B, Ci, H, W in WGRAD_SIZES:
        g = torch.Generator().manual_seed(B + H)
        x, dc = torch.randn((B, Ci, H, W), generator=g).to(dev), torch.randn((B, 1, H, W), generator=g).to(dev)
        code, detail = ops.conv_wgrad_plan(_lib.DEFINES["DMB_WGRAD_2D"], x, dc, 3, 1)
        res = dict(workload="wgrad_c1_2d", x=[B, Ci, H, W], plan="0x%03x" % code, detail=list(detail), library=os.path.basename(_lib.LIB_PATH),
                   binding=binding)
        _put(res, "hip", timed(lambda: ops.conv2d_wgrad(x, dc, 3, 1), args.iters, args.repeats))
        res["gflops"] = 2.0 * B * H * W * Ci * 9 / 1e6 / res["hip_ms"]
        _put(res, "stock", timed(lambda: torch.nn.grad.conv2d_weight(x, (1, Ci, 3, 3), dc, stride=1, padding=1), args.iters, args.repeats))
        res["speedup_vs_stock"] = res["stock_ms"] / res["hip_ms"]
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    return lines


def _stage_inputs(cfg, B, dev):
    planes, (H, W) = CONFIGS[cfg]
    g = torch.Generator().manual_seed(10 * B + len(planes))
    fms = [torch.randn((B, planes[i] - 1, H << i, W << i), generator=g).to(dev).requires_grad_() for i in range(len(planes))]
    return torch.randn((B, 1, H, W), generator=g).to(dev).requires_grad_(), fms


def stages(args, dev):
    from densematchingbenchmark_amd.modeling.stereo.disp_refinement import DeepPrunerRefinement
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    from tests import _deeppruner_features_ref as R
    lines, slower, stage_ms = [], False, {}
    for cfg, (planes, hw) in CONFIGS.items():
        for B in (1, 4):
            hip_mod = R.seeded_state(DeepPrunerRefinement(list(planes), True, len(planes)), 7).to(dev).train()
            ref_mod = R.seeded_state(R.DeepPrunerRefinement(list(planes), True, len(planes)), 7).to(dev).train()
            disp, fms = _stage_inputs(cfg, B, dev)
            with torch.no_grad():
                ups = [torch.randn_like(o) for o in ref_mod([disp], fms)[:-1]]
            hp, rp = list(hip_mod.parameters()), list(ref_mod.parameters())

            def hip():
                return torch.autograd.grad(train_fn.deeppruner_refinement(hip_mod, [disp], fms)[:-1], [disp] + fms + hp, ups)

            def stock():
                return torch.autograd.grad(ref_mod([disp], fms)[:-1], [disp] + fms + rp, ups)
            res = dict(workload="deeppruner_refinement_fwd_bwd", config=cfg, batch=B, guides=[[B, p] + [hw[0] << i, hw[1] << i] for i, p in enumerate(planes)])
            _put(res, "hip", timed(hip, args.iters, args.repeats))
            _put(res, "stock", timed(stock, args.iters, args.repeats))
            res["speedup"] = res["stock_ms"] / res["hip_ms"]
            stage_ms[(cfg, B)] = res["hip_ms"]
            lines.append(json.dumps(res))
            slower = slower or res["speedup"] <= 1.0
            print(lines[-1], flush=True)
            del hip_mod, ref_mod, disp, fms, ups
            torch.cuda.empty_cache()
    return lines, slower, stage_ms


def tails(args, dev, stage_ms):
    from densematchingbenchmark_amd.modeling.stereo.disp_refinement import RefinementHeand
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    lines = []
    for cfg, (planes, (H, W)) in CONFIGS.items():
        for B in (1, 4):
            res = dict(workload="refinement_head_fwd_bwd", config=cfg, batch=B, tails=[])
            total = 0.0
            for i in range(len(planes)):
                h, w = H << i, W << i
                block = RefinementHeand(planes[i]).to(dev)
                x = torch.randn((B, 16, h, w), device=dev, requires_grad=True)
                init = torch.randn((B, 1, h, w), device=dev, requires_grad=True)
                up = torch.randn((B, 1, 2 * h, 2 * w), device=dev)
                wt = block.classify.weight

                def tail():
                    return torch.autograd.grad(train_fn.refinement_head(block, init, x), [x, init, wt], up)
                one = dict(x=[B, 16, h, w])
                _put(one, "fwd_bwd", timed(tail, args.iters, args.repeats))
                dc = torch.randn((B, 1, h, w), device=dev)
                wd = wt.detach()
                _put(one, "dgrad_preact_conv", timed(lambda: ops.preact_conv(dc, wd.flip(2, 3).transpose(0, 1).contiguous()), args.iters, args.repeats))
                _put(one, "dgrad_conv2d_dgrad", timed(lambda: ops.conv2d_dgrad(dc, wd), args.iters, args.repeats))
                _put(one, "wgrad", timed(lambda: ops.conv2d_wgrad(x.detach(), dc, 3, 1), args.iters, args.repeats))
                total += one["fwd_bwd_ms"]
                res["tails"].append(one)
            res["tail_ms"] = total
            if (cfg, B) in stage_ms:
                res["stage_hip_ms"] = stage_ms[(cfg, B)]
                res["tail_share"] = total / stage_ms[(cfg, B)]
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("wgrad", "stages", "tail"), default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = wgrads(args, dev) if args.only in (None, "wgrad") else []
    more, slower, stage_ms = stages(args, dev) if args.only in (None, "stages") else ([], False, {})
    lines += more
    if args.only in (None, "tail"):
        lines += tails(args, dev, stage_ms)
    if args.out and lines:
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")
    if slower:
        sys.exit("forward + backward of the HIP refinement path is not faster than stock autograd at every measured config and batch")


if __name__ == "__main__":
    main()
