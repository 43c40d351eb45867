"""DeepPruner's cost processor on one GPU: the HIP path (csrc/deeppruner_heads.hip, csrc/conv3d_hw.hip and the stride-1 kernels of
conv3d.hip) against stock PyTorch-ROCm running the plain ``torch.nn`` restatement (tests/_deeppruner_processor_ref.py) with the
same weights on the SAME GPU, at the feature sizes of the 4x config's evaluation and KITTI shapes (C = 32, P = 14, N = 9).  One
JSON line per measurement:

  deeppruner_processor         per (size, batch): ms per pre + post call -- HIP eager, HIP replayed from a captured graph, stock --
                               and the stock / HIP ratio.                                         GATE: HIP faster at every row.
  deeppruner_volume            the post form [B, 93, 9, H, W] against the composition it replaces (``ops.fast_cat_fms`` + two
                               ``torch.cat``), and the achieved GB/s on the bytes it must move (the output once plus the inputs)
                               next to ``ops.fast_cat_fms`` alone on its 64 channels.             GATE: faster at every row.
  conv2d_k5_small              14 -> 14 on 136 x 240, 9 -> 9 on 272 x 480 and 1 -> 1 on both against ``F.conv2d``: reported
                               whatever it shows.
  deeppruner_processor_census  batch 1: launches per stage (as the module's docstring counts them) and the share of the pre
                               stage's time spent in the two (hourglass, 16 -> 32, 32 -> 1) branches.

Each figure is the median of ``--repeats`` HIP-event timings of ``--iters`` back-to-back calls, after a warm-up.  Non-zero exit if a
gate fails.

    python scripts/bench_deeppruner_processor.py [--iters 10] [--repeats 5] [--out profiles/deeppruner_processor_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from densematchingbenchmark_amd import ops, ops_deeppruner  # noqa: E402
from densematchingbenchmark_amd.config import Config  # noqa: E402
from densematchingbenchmark_amd.modeling.stereo.cost_processors.DeepPruner import DeepPrunerProcessor  # noqa: E402
from tests import _deeppruner_processor_ref as R  # noqa: E402

SIZES = ((136, 240), (96, 312))           # H/4 x W/4 of 544x960 and of 384x1248
C, P, N = 32, 14, 9
HBM_PEAK_GBS = 8000.0                     # the MI355X's specified HBM3E peak


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


def _cfg():
    return Config(dict(model=dict(batch_norm=True, cost_processor=dict(
        type="DeepPruner", patch_match_disparity_sample_number=P, uniform_disparity_sample_number=N,
        confidence_range_predictor=dict(in_planes=2 * C + 1, hourglass_in_planes=16),
        cost_aggregator=dict(type="DeepPruner", in_planes=2 * C + 2 * P + 1, hourglass_in_planes=16)))))


def inputs(B, H, W, dev):
    g = torch.Generator().manual_seed(H + B)
    left, right = torch.randn((B, C, H, W), generator=g), torch.randn((B, C, H, W), generator=g)
    pre = torch.sort(torch.rand((B, P, H, W), generator=g) * 48.0, dim=1)[0]
    post = torch.sort(torch.rand((B, N, H, W), generator=g) * 48.0, dim=1)[0]
    return tuple(t.to(dev) for t in (left, right, pre, post))


def both_stages(proc, left, right, pre, post):
    a = proc("pre", left, right, pre)
    return list(a) + list(proc("post", left, right, post, a[2], a[3]))


def volume_row(B, H, W, dev, iters, repeats):
    left, right, _, post = inputs(B, H, W, dev)
    fmin, fmax = torch.randn((B, P, H, W), device=dev), torch.randn((B, P, H, W), device=dev)

    def composed():
        raw = torch.cat((ops.fast_cat_fms(left, right, post), post.unsqueeze(1)), 1)
        return torch.cat((raw, fmin.unsqueeze(2).expand(-1, -1, N, -1, -1), fmax.unsqueeze(2).expand(-1, -1, N, -1, -1)), 1)

    fused = lambda: ops_deeppruner.deeppruner_volume(left, right, post, fmin, fmax)                 # noqa: E731
    cat_only = lambda: ops.fast_cat_fms(left, right, post)                                          # noqa: E731
    assert torch.equal(fused(), composed())
    res = dict(workload="deeppruner_volume", output=[B, 2 * C + 1 + 2 * P, N, H, W])
    res["fused_us"] = 1e3 * timed(fused, iters, repeats)
    res["composition_us"] = 1e3 * timed(composed, iters, repeats)
    res["fast_cat_fms_us"] = 1e3 * timed(cat_only, iters, repeats)
    res["speedup"] = res["composition_us"] / res["fused_us"]
    plane = 4 * B * H * W
    must = plane * ((2 * C + 1 + 2 * P) * N + 2 * C + N + 2 * P)          # the output once, plus L, R, the samples and both features
    must_cat = plane * (2 * C * N + 2 * C + N)
    res["fused_gbs"], res["fast_cat_fms_gbs"] = must / res["fused_us"] / 1e3, must_cat / res["fast_cat_fms_us"] / 1e3
    res["fused_share_of_hbm_peak"] = res["fused_gbs"] / HBM_PEAK_GBS
    res["fast_cat_fms_share_of_hbm_peak"] = res["fast_cat_fms_gbs"] / HBM_PEAK_GBS
    return res


def conv_row(Ci, H, W, dev, iters, repeats):
    g = torch.Generator().manual_seed(Ci + H)
    x = torch.randn((1, Ci, H, W), generator=g).to(dev)
    w = (torch.randn((Ci, Ci, 5, 5), generator=g) / (Ci * 25) ** 0.5).to(dev)
    scale, shift = (torch.rand((Ci,), generator=g) + 0.5).to(dev), (torch.rand((Ci,), generator=g) - 0.5).to(dev)
    hip = lambda: ops_deeppruner.conv2d_k5_small(x, w, scale, shift, True)                                         # noqa: E731
    # stock gets the affine folded into its weights and bias: one library call, the cheapest form stock torch has
    ws = w * scale.view(-1, 1, 1, 1)
    stock = lambda: F.relu_(F.conv2d(x, ws, shift, stride=1, padding=2))                                           # noqa: E731
    res = dict(workload="conv2d_k5_small", channels=[Ci, Ci], input=[1, Ci, H, W], max_abs_diff=(hip() - stock()).abs().max().item())
    res["hip_us"] = 1e3 * timed(hip, iters, repeats)
    res["stock_us"] = 1e3 * timed(stock, iters, repeats)
    res["speedup"] = res["stock_us"] / res["hip_us"]
    return res


def census(proc, H, W, dev, iters, repeats):
    """Batch 1: launches per stage (every unit is one launch: cost_processors/DeepPruner.py's docstring) and the pre stage's time
    inside the two range branches."""
    left, right, pre, post = inputs(1, H, W, dev)
    crp = proc.confidence_range_predictor
    raw = ops_deeppruner.deeppruner_volume(left, right, pre)
    trunk = crp.dres1(crp.dres0(raw))
    branches = lambda: (crp.min_disparity_predictor(trunk), crp.max_disparity_predictor(trunk))        # noqa: E731
    stage = lambda: proc("pre", left, right, pre)                                                       # noqa: E731
    feats = stage()
    post_stage = lambda: proc("post", left, right, post, feats[2], feats[3])                            # noqa: E731
    res = dict(workload="deeppruner_processor_census", features=[1, C, H, W], launches_pre=1 + 4 + 2 * 11 + 2 + 4,
               launches_post=1 + 14 + 1 + 2 + 2)
    res["pre_ms"], res["post_ms"] = timed(stage, iters, repeats), timed(post_stage, iters, repeats)
    res["pre_branches_ms"] = timed(branches, iters, repeats)
    res["pre_branches_share"] = res["pre_branches_ms"] / res["pre_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines, failed = [], []

    def emit(res):
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

    with torch.no_grad():
        hip_proc = R.seeded_state(DeepPrunerProcessor(_cfg()), 5).to(dev).eval()
        stock_proc = R.seeded_state(R.DeepPrunerProcessor(C, P, N), 5).to(dev).eval()
        for H, W in SIZES:
            for B in (1, 4):
                x = inputs(B, H, W, dev)
                hip = lambda: both_stages(hip_proc, *x)                                               # noqa: E731
                stock = lambda: both_stages(stock_proc, *x)                                           # noqa: E731
                # the outputs are compared from the SAME volumes (the HIP path's, bit-identical to the reference's on the CPU): stock
                # torch's grid_sample on the GPU rounds the warp differently, and where T ~ 0 that flips the mask of the left features
                a = hip()
                b = list(stock_proc.from_volume("pre", ops_deeppruner.deeppruner_volume(*x[:3]), x[2]))
                b += stock_proc.from_volume("post", ops_deeppruner.deeppruner_volume(x[0], x[1], x[3], a[2], a[3]), x[3])
                res = dict(workload="deeppruner_processor", features=[B, C, H, W], samples=[P, N],
                           max_abs_diff=[(u - v).abs().max().item() for u, v in zip(a, b)], max_abs=[v.abs().max().item() for v in b])
                del a, b
                res["hip_ms"] = timed(hip, args.iters, args.repeats)
                res["hip_graph_ms"] = timed(graphed(hip), args.iters, args.repeats)
                res["stock_ms"] = timed(stock, max(3, args.iters // 2), args.repeats)
                res["speedup"] = res["stock_ms"] / res["hip_ms"]
                emit(res)
                if res["speedup"] <= 1.0:
                    failed.append("processor %s" % res["features"])
                row = volume_row(B, H, W, dev, args.iters, args.repeats)
                emit(row)
                if row["speedup"] <= 1.0:
                    failed.append("volume %s" % row["output"])
        for Ci, (H, W) in ((14, SIZES[0]), (9, (2 * SIZES[0][0], 2 * SIZES[0][1])), (1, SIZES[0]), (1, (2 * SIZES[0][0], 2 * SIZES[0][1]))):
            emit(conv_row(Ci, H, W, dev, args.iters, args.repeats))
        for H, W in SIZES:
            emit(census(hip_proc, H, W, dev, args.iters, args.repeats))
    if args.out and lines:
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")
    if failed:
        sys.exit("the HIP path is not faster at: " + "; ".join(failed))


if __name__ == "__main__":
    main()
