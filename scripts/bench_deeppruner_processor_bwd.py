"""Forward plus backward of DeepPruner's cost processor on one GPU: the HIP path (train_fn.deeppruner_processor, both stages, at
features [B, 32, 64, 128] with P = 14 PatchMatch samples and N = 9 uniform samples: a 256 x 512 training crop of the 4x config)
against stock PyTorch-ROCm autograd through the restatement (tests/_deeppruner_processor_ref.py) with the same weights on the SAME
GPU, batch 1 and 4, modules in train().  One JSON line per stage and batch: ms per forward + backward, the stock / HIP ratio and the
peak memory either path adds.  Then, alone:
  * the six 5x5 weight-gradient launches of those passes (csrc/wgrad.hip, plan form 6) against torch.nn.grad.conv2d_weight;
  * the composed soft-arg-min backward (SoftArgminSampledFn) and the composed volume backward (DeepPrunerVolumeFn), each with its
    share of its stage's forward + backward.

Each figure is the median of ``--repeats`` HIP-event timings of ``--iters`` back-to-back calls, after a warm-up.  Exits non-zero
unless the HIP path is faster than stock at every measured stage and batch (the tables of single launches carry no threshold).

    python scripts/bench_deeppruner_processor_bwd.py [--iters 10] [--repeats 5] [--out profiles/deeppruner_processor_bwd_bench.jsonl]
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
from densematchingbenchmark_amd.config import Config  # noqa: E402
from densematchingbenchmark_amd.modeling.stereo.cost_processors.DeepPruner import DeepPrunerProcessor  # noqa: E402
from densematchingbenchmark_amd.modeling.stereo.layers import train_fn  # noqa: E402
from tests import _deeppruner_processor_ref as R  # noqa: E402

C, P, N, H, W = 32, 14, 9, 64, 128
# the six launches: (stage, layer, channels, H, W)
WGRAD_LAUNCHES = [("pre", "min_disparity_conv", 1, H, W), ("pre", "max_disparity_conv", 1, H, W),
                  ("pre", "min_disparity_feature_conv", P, H, W), ("pre", "max_disparity_feature_conv", P, H, W),
                  ("post", "disparity_conv", 1, 2 * H, 2 * W), ("post", "disparity_feature_conv", N, 2 * H, 2 * W)]


def _cfg():
    return Config(dict(model=dict(batch_norm=True, cost_processor=dict(
        type="DeepPruner", patch_match_disparity_sample_number=P, uniform_disparity_sample_number=N,
        confidence_range_predictor=dict(in_planes=2 * C + 1, hourglass_in_planes=R.HOURGLASS_IN_PLANES),
        cost_aggregator=dict(type="DeepPruner", in_planes=2 * C + 2 * P + 1, hourglass_in_planes=R.HOURGLASS_IN_PLANES)))))


def _inputs(stage, B, dev):
    g = torch.Generator().manual_seed(100 * B + (0 if stage == "pre" else 1))
    D = P if stage == "pre" else N
    t = [torch.randn((B, C, H, W), generator=g), torch.randn((B, C, H, W), generator=g),
         torch.sort(torch.rand((B, D, H, W), generator=g) * (W / 2.0), dim=1)[0]]
    if stage == "post":
        t += [torch.rand((B, P, H, W), generator=g), torch.rand((B, P, H, W), generator=g)]
    return [v.to(dev).requires_grad_() for v in t]


def stages(args, dev):
    lines, slower, stage_ms = [], False, {}
    for stage in ("pre", "post"):
        for B in (1, 4):
            hip_mod = R.seeded_state(DeepPrunerProcessor(_cfg()), 7).to(dev).train()
            ref_mod = R.seeded_state(R.DeepPrunerProcessor(C, P, N), 7).to(dev).train()
            x = _inputs(stage, B, dev)
            with torch.no_grad():
                ups = [torch.randn_like(o) for o in ref_mod(stage, *x)]
            # the parameters the stage uses
            used = "confidence_range_predictor." if stage == "pre" else ("cost_aggregator.", "disparity_conv.", "disparity_feature_conv.")
            hp = [p for k, p in hip_mod.named_parameters() if k.startswith(used)]
            rp = [p for k, p in ref_mod.named_parameters() if k.startswith(used)]

            def hip():
                return torch.autograd.grad(list(train_fn.deeppruner_processor(hip_mod, stage, *x)), x + hp, ups)

            def stock():
                return torch.autograd.grad(list(ref_mod(stage, *x)), x + rp, ups)
            res = dict(workload="deeppruner_processor_%s_fwd_bwd" % stage, features=[B, C, H, W], samples=P if stage == "pre" else N, batch=B)
            res["hip_ms"] = timed(hip, args.iters, args.repeats)
            res["hip_peak_mb"] = peak_rise(hip)
            res["stock_ms"] = timed(stock, args.iters, args.repeats)
            res["stock_peak_mb"] = peak_rise(stock)
            res["speedup"] = res["stock_ms"] / res["hip_ms"]
            stage_ms[(stage, B)] = res["hip_ms"]
            lines.append(json.dumps(res))
            slower = slower or res["speedup"] <= 1.0
            print(lines[-1], flush=True)
            del hip_mod, ref_mod, x, ups
            torch.cuda.empty_cache()
    return lines, slower, stage_ms


def wgrads(args, dev):
    lines = []
    for stage, layer, ch, h, w in WGRAD_LAUNCHES:
        for B in (1, 4):
            g = torch.Generator().manual_seed(ch + B + h)
            x, dc = torch.randn((B, ch, h, w), generator=g).to(dev), torch.randn((B, ch, h, w), generator=g).to(dev)
            code, detail = ops.conv_wgrad_plan(_lib.DEFINES["DMB_WGRAD_2D"], x, dc, 5, 1)
            res = dict(workload="wgrad_k5", stage=stage, layer=layer, x=list(x.shape), plan="0x%03x" % code, detail=list(detail))
            res["hip_ms"] = timed(lambda: ops.conv2d_wgrad(x, dc, 5, 1), args.iters, args.repeats)
            res["gflops"] = 2.0 * B * h * w * ch * ch * 25 / 1e6 / res["hip_ms"]
            res["stock_ms"] = timed(lambda: torch.nn.grad.conv2d_weight(x, (ch, ch, 5, 5), dc, stride=1, padding=2), args.iters, args.repeats)
            res["speedup"] = res["stock_ms"] / res["hip_ms"]
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    return lines


def composed(args, dev, stage_ms):
    """The two backwards that are compositions of existing launches and torch element-wise ops, alone"""
    lines = []
    for stage in ("pre", "post"):
        for B in (1, 4):
            x = _inputs(stage, B, dev)
            D = x[2].shape[1]
            cost = torch.randn((B, D, H, W), device=dev, requires_grad=True)
            disp = train_fn.SoftArgminSampledFn.apply(cost, x[2])
            up = torch.randn_like(disp)
            vol = train_fn.deeppruner_volume(*x)
            upv = torch.randn_like(vol)
            res = dict(workload="composed_backwards", stage=stage, batch=B, samples=D, volume=list(vol.shape))
            res["soft_argmin_bwd_ms"] = timed(lambda: torch.autograd.grad(disp, [cost, x[2]], up, retain_graph=True), args.iters, args.repeats)
            res["soft_argmin_calls"] = 2 if stage == "pre" else 1
            res["volume_bwd_ms"] = timed(lambda: torch.autograd.grad(vol, x, upv, retain_graph=True), args.iters, args.repeats)
            if (stage, B) in stage_ms:
                res["stage_hip_ms"] = stage_ms[(stage, B)]
                res["soft_argmin_share"] = res["soft_argmin_calls"] * res["soft_argmin_bwd_ms"] / stage_ms[(stage, B)]
                res["volume_share"] = res["volume_bwd_ms"] / stage_ms[(stage, B)]
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
            del x, cost, disp, vol, up, upv
            torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("stages", "wgrad", "composed"), default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines, slower, stage_ms = stages(args, dev) if args.only in (None, "stages") else ([], False, {})
    if args.only in (None, "wgrad"):
        lines += wgrads(args, dev)
    if args.only in (None, "composed"):
        lines += composed(args, dev, stage_ms)
    if args.out and lines:
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")
    if slower:
        sys.exit("forward + backward of the HIP processor path is not faster than stock autograd at every measured stage and batch")


if __name__ == "__main__":
    main()
