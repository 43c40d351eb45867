"""Forward plus backward of DeepPruner's aggregator and of its hourglass on one GPU: the HIP path (train_fn.deeppruner_aggregator at
[B, 93, 9, 64, 128] and train_fn.hw_hourglass at [B, 16, 14, 64, 128], the volumes of a 256 x 512 training crop of the 4x config)
against stock PyTorch-ROCm autograd through the restatement (tests/_hw_ref.py) with the same weights on the SAME GPU, batch 1 and 4,
modules in train().  One JSON line per workload and batch: ms per forward + backward, the stock / HIP ratio and the peak memory
either path adds.  Then one line per stride-(1, 2, 2) weight-gradient launch of those passes alone (csrc/wgrad.hip, plan form 5)
against torch.nn.grad.conv3d_weight on the same GPU, with its share of the FP32 matrix peak; ``--segments`` adds the same launch with
the number of z segments forced (the development library, DMB_LIB=dev): what WG_SEG_HW of csrc/wgrad_plan.h was fitted on.

Each figure is the median of ``--repeats`` HIP-event timings of ``--iters`` back-to-back calls, after a warm-up.  Exits non-zero
unless the HIP path is faster than stock at every measured workload and batch (the weight-gradient table carries no threshold).

    python scripts/bench_deeppruner_aggregator_bwd.py [--iters 10] [--repeats 5] [--out profiles/deeppruner_aggregator_bwd_bench.jsonl]
    DMB_LIB=dev python scripts/bench_deeppruner_aggregator_bwd.py --segments --only wgrad
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_deeppruner_sampler import timed  # noqa: E402
from bench_deeppruner_sampler_bwd import peak_rise  # noqa: E402
from densematchingbenchmark_amd import _lib, ops  # noqa: E402
from densematchingbenchmark_amd.modeling.stereo.cost_processors.aggregators import DeepPrunerAggregator  # noqa: E402
from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils import HWHourglass  # noqa: E402
from densematchingbenchmark_amd.modeling.stereo.layers import train_fn  # noqa: E402
from tests import _hw_ref as R  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3     # v_mfma_f32_32x32x2_f32, dense (bench.py)
# the six launches: (role, small channels, big channels, small H, small W); D and B vary
WGRAD_LAUNCHES = [("conv 16 -> 32", 32, 16, 32, 64), ("conv 32 -> 64", 64, 32, 16, 32), ("conv 64 -> 128", 128, 64, 8, 16),
                  ("transposed 128 -> 64", 128, 64, 8, 16), ("transposed 64 -> 32", 64, 32, 16, 32), ("transposed 32 -> 16", 32, 16, 32, 64)]


def networks(args, dev):
    lines, slower = [], False
    for what, planes, D in (("deeppruner_aggregator", 93, 9), ("hw_hourglass", 16, 14)):
        for B in (1, 4):
            g = torch.Generator().manual_seed(planes + B)
            x = torch.randn((B, planes, D, 64, 128), generator=g).to(dev).requires_grad_()
            if what == "hw_hourglass":
                hip_mod, ref_mod = HWHourglass(16), R.HWHourglass(16)
                up = torch.randn((B, 16, D, 64, 128), generator=g).to(dev)
                fwd = train_fn.hw_hourglass
            else:
                hip_mod, ref_mod = DeepPrunerAggregator(planes, 16), R.DeepPrunerAggregator(planes, 16)
                up = torch.randn((B, D, 64, 128), generator=g).to(dev)
                fwd = lambda m, t: train_fn.deeppruner_aggregator(m, t)[0]      # noqa: E731
            hip_mod, ref_mod = R.seeded_state(hip_mod, 7).to(dev).train(), R.seeded_state(ref_mod, 7).to(dev).train()
            hp, rp = list(hip_mod.parameters()), list(ref_mod.parameters())

            def hip():
                return torch.autograd.grad(fwd(hip_mod, x), [x] + hp, up)

            def stock():
                out = ref_mod(x)
                return torch.autograd.grad(out[0] if isinstance(out, list) else out, [x] + rp, up)
            res = dict(workload=what + "_fwd_bwd", shape=list(x.shape), batch=B)
            res["hip_ms"] = timed(hip, args.iters, args.repeats)
            res["hip_peak_mb"] = peak_rise(hip)
            res["stock_ms"] = timed(stock, args.iters, args.repeats)
            res["stock_peak_mb"] = peak_rise(stock)
            res["speedup"] = res["stock_ms"] / res["hip_ms"]
            lines.append(json.dumps(res))
            slower = slower or res["speedup"] <= 1.0
            print(lines[-1], flush=True)
            del hip_mod, ref_mod, x, up
            torch.cuda.empty_cache()
    return lines, slower


def wgrads(args, dev):
    lines = []
    for role, Cs, Cb, H, W in WGRAD_LAUNCHES:
        for B, D in ((1, 9), (4, 9), (1, 14), (4, 14)):
            g = torch.Generator().manual_seed(Cs + B + D)
            small, big = torch.randn((B, Cs, D, H, W), generator=g).to(dev), torch.randn((B, Cb, D, 2 * H, 2 * W), generator=g).to(dev)
            code, detail = ops.conv_wgrad_plan(_lib.DEFINES["DMB_WGRAD_S2"], small, big)
            gflop = 2.0 * B * D * H * W * Cs * Cb * 27 / 1e9
            res = dict(workload="wgrad_hw", launch=role, small=list(small.shape), big=list(big.shape), plan="0x%03x" % code, detail=list(detail))
            # (both roles are the same sum: small = dc and big = x of the convolution, small = x and big = dy of the transposed one)
            res["hip_ms"] = timed(lambda: ops.conv3d_k3s2_wgrad(big, small), args.iters, args.repeats)
            res["frac_fp32_peak"] = gflop / res["hip_ms"] / PEAK_FP32_MFMA_TFLOPS
            res["stock_ms"] = timed(lambda: torch.nn.grad.conv3d_weight(big, (Cs, Cb, 3, 3, 3), small, stride=(1, 2, 2), padding=1),
                                    args.iters, args.repeats)
            if args.segments:
                res["ms_by_segments"] = {}
                for nseg in [n for n in (1, 2, 3, 5, 7, D) if n <= D]:
                    _lib.load().dmb_dev_set_option(5, nseg)
                    res["ms_by_segments"][nseg] = timed(lambda: ops.conv3d_k3s2_wgrad(big, small), args.iters, args.repeats)
                _lib.load().dmb_dev_set_option(5, 0)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("networks", "wgrad"), default=None)
    ap.add_argument("--segments", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines, slower = ([], False) if args.only == "wgrad" else networks(args, dev)
    if args.only != "networks":
        lines += wgrads(args, dev)
    if args.out and lines:
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")
    if slower:
        sys.exit("forward + backward of the HIP aggregator path is not faster than stock autograd at every measured shape")


if __name__ == "__main__":
    main()
