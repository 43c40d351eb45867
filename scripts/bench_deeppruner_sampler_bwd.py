"""Forward plus backward of DeepPruner's sampler, stage "pre", on one GPU: the HIP path (train_fn.deeppruner_sampler on
csrc/patch_match.hip, eager and replayed from a captured graph) against stock PyTorch-ROCm autograd through the functional
restatement (tests/_deeppruner_ref.py) on the SAME GPU, at the feature sizes of the reference's two DeepPruner configs, batch 1
and 4.  One JSON line per size and batch: ms per forward + backward and the stock / HIP ratio, and the peak memory either path
adds.  Each figure is the median of ``--repeats`` HIP-event timings of ``--iters`` back-to-back calls, after a warm-up.  Exits
non-zero unless the HIP path is faster at every measured size and batch.

    python scripts/bench_deeppruner_sampler_bwd.py [--iters 20] [--repeats 5] [--out profiles/deeppruner_sampler_bwd_bench.jsonl]
    python scripts/bench_deeppruner_sampler_bwd.py --trace      # a few calls of the HIP path only, for a kernel trace
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_deeppruner_sampler import SIZES, graphed, timed  # noqa: E402
from densematchingbenchmark_amd.modeling.stereo.disp_samplers import DeepPrunerSampler  # noqa: E402
from densematchingbenchmark_amd.modeling.stereo.layers import train_fn  # noqa: E402
from tests import _deeppruner_ref as R  # noqa: E402


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines, slower = [], False
    for H, W, max_disp in SIZES:
        for B in (1,) if args.trace else (1, 4):
            g = torch.Generator().manual_seed(H + B)
            left, right = (torch.randn((B, 32, H, W), generator=g).to(dev).requires_grad_() for _ in range(2))
            noise = torch.rand((B, 12, H, W), generator=g).to(dev)
            up = torch.randn((B, 14, H, W), generator=g).to(dev)
            s = DeepPrunerSampler(max_disp=max_disp).eval()

            def hip():
                return torch.autograd.grad(train_fn.deeppruner_sampler(s, 'pre', left, right, noise=noise), (left, right), up)

            def stock():
                return torch.autograd.grad(R.sampler('pre', left, right, noise=noise, max_disp=max_disp), (left, right), up)
            if args.trace:
                for _ in range(5):
                    hip()
                torch.cuda.synchronize()
                continue
            res = dict(workload="deeppruner_sampler_fwd_bwd", size=[H, W], max_disp=max_disp, batch=B, channels=32)
            res["hip_ms"] = timed(hip, args.iters, args.repeats)
            res["hip_graph_ms"] = timed(graphed(hip), args.iters, args.repeats)
            res["hip_peak_mb"] = peak_rise(hip)
            res["stock_ms"] = timed(stock, args.iters, args.repeats)
            res["stock_peak_mb"] = peak_rise(stock)
            res["speedup"] = res["stock_ms"] / res["hip_ms"]
            lines.append(json.dumps(res))
            slower = slower or res["speedup"] <= 1.0
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    if args.out and lines:
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")
    if slower:
        sys.exit("forward + backward of the HIP \"pre\" stage is not faster than stock autograd at every measured shape")


if __name__ == "__main__":
    main()
