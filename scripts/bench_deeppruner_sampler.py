"""DeepPruner's disparity sampler on one GPU: the HIP path (csrc/patch_match.hip) against stock PyTorch-ROCm running the
functional restatement (tests/_deeppruner_ref.py: shifts, a 5-D grid_sample, a channel mean and a softmax per half-iteration) on
the SAME GPU, at the feature sizes of the reference's two DeepPruner configs.  For each size and batch prints one JSON line: ms per
call of stage "pre" (eager, and the HIP path replayed from a captured graph) and of stage "post", and the stock / HIP ratios.
Each figure is the median of ``--repeats`` HIP-event timings of ``--iters`` back-to-back calls, after a warm-up.

    python scripts/bench_deeppruner_sampler.py [--iters 20] [--repeats 5] [--out profiles/deeppruner_sampler_bench.jsonl]
    python scripts/bench_deeppruner_sampler.py --trace      # a few calls of the HIP path only, for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from densematchingbenchmark_amd.modeling.stereo.disp_samplers import DeepPrunerSampler  # noqa: E402
from tests import _deeppruner_ref as R  # noqa: E402

SIZES = ((136, 240, 48), (68, 120, 24))     # H/4 x W/4 of 544x960 with max_disp 48 (4x config), H/8 x W/8 with 24 (8x config)


def timed(fn, iters, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return statistics.median(ms)


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines, slower = [], False
    with torch.no_grad():
        for H, W, max_disp in SIZES:
            for B in (1, 4):
                g = torch.Generator().manual_seed(H + B)
                left, right = (torch.randn((B, 32, H, W), generator=g).to(dev) for _ in range(2))
                noise = torch.rand((B, 12, H, W), generator=g).to(dev)
                lo = (torch.rand((B, 1, H, W), generator=g) * max_disp).to(dev)
                hi = lo + (torch.rand((B, 1, H, W), generator=g) * 20.0 - 4.0).to(dev)
                s = DeepPrunerSampler(max_disp=max_disp).eval()
                hip_pre = lambda: s('pre', left, right, noise=noise)                                  # noqa: E731
                hip_post = lambda: s('post', left, right, lo, hi)                                     # noqa: E731
                if args.trace:
                    for _ in range(5):
                        hip_pre()
                        hip_post()
                    torch.cuda.synchronize()
                    continue
                stock_pre = lambda: R.sampler('pre', left, right, noise=noise, max_disp=max_disp)     # noqa: E731
                stock_post = lambda: R.sampler('post', left, right, lo, hi, max_disp=max_disp)        # noqa: E731
                res = dict(workload="deeppruner_sampler", size=[H, W], max_disp=max_disp, batch=B, channels=32)
                res["hip_pre_ms"] = timed(hip_pre, args.iters, args.repeats)
                res["hip_pre_graph_ms"] = timed(graphed(hip_pre), args.iters, args.repeats)
                res["stock_pre_ms"] = timed(stock_pre, max(3, args.iters // 4), args.repeats)
                res["pre_speedup"] = res["stock_pre_ms"] / res["hip_pre_ms"]
                res["hip_post_ms"] = timed(hip_post, args.iters, args.repeats)
                res["stock_post_ms"] = timed(stock_post, args.iters, args.repeats)
                res["post_speedup"] = res["stock_post_ms"] / res["hip_post_ms"]
                lines.append(json.dumps(res))
                slower = slower or res["pre_speedup"] <= 1.0
                print(lines[-1], flush=True)
    if args.out and lines:
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")
    if slower:
        sys.exit("the HIP \"pre\" stage is not faster than stock torch at every measured shape")


if __name__ == "__main__":
    main()
