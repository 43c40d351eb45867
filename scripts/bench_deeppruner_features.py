"""DeepPruner's refinement and backbones on one GPU: the HIP path (csrc/refine_head.hip and the fused conv2d kernel) against what it
replaces and against stock PyTorch-ROCm running the plain ``torch.nn`` restatement (tests/_deeppruner_features_ref.py) with the
same weights on the SAME GPU.  One JSON line per measurement:

  refine_head                  the fused tail against the two launches it replaces (``ops.conv2d`` with one output channel, residual
                               and ReLU, then ``ops.bilinear_scale`` with mult 2) at Ci = 16, [1|4, 16, 272, 480] and
                               [1|4, 16, 136, 240]; GB/s on the bytes that must move (x, init and the output once) and the
                               composition's own run-to-run spread (max - min of its repeats).
                               GATE: faster at every row by more than that spread.
  deeppruner_refinement        ``DeepPrunerRefinement`` at both configs' shapes (4x: one stage at 272 x 480; 8x: 136 x 240 then
                               272 x 480), batch 1 and 4 -- HIP eager, HIP replayed from a captured graph, stock -- and the
                               stock / HIP ratio.                                                 GATE: HIP faster at every row.
  deeppruner_refinement_census batch 1, the 4x stage: launches, and per layer the HIP and the stock time.
  deeppruner_backbone          both backbones at [1|4, 3, 544, 960], two views per call, HIP eager against stock.
                                                                                                  GATE: HIP faster at every row.
  stride2_64to128              the two-launch stride-2 64 -> 128 layers of the fast backbone's layer3 (3x3 and 1x1, on
                               [1|4, 64, 136, 240]) next to the single stock layer: reported whatever it shows.

Each figure is the median of ``--repeats`` HIP-event timings of ``--iters`` back-to-back calls, after a warm-up.  Non-zero exit if a
gate fails.

    python scripts/bench_deeppruner_features.py [--iters 10] [--repeats 5] [--out profiles/deeppruner_features_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from densematchingbenchmark_amd import ops, ops_deeppruner  # noqa: E402
from densematchingbenchmark_amd.modeling.stereo.backbones import DeepPrunerBestBackbone, DeepPrunerFastBackbone  # noqa: E402
from densematchingbenchmark_amd.modeling.stereo.disp_refinement import DeepPrunerRefinement  # noqa: E402
from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers_2d import FusedConv2d  # noqa: E402
from tests import _deeppruner_features_ref as R  # noqa: E402

HALF, QUARTER = (272, 480), (136, 240)    # H/2 x W/2 and H/4 x W/4 of 544 x 960
HBM_PEAK_GBS = 8000.0                     # the MI355X's specified HBM3E peak


def timings(fn, iters, repeats, warmup=3):
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
    return ms


def timed(fn, iters, repeats, warmup=3):
    return statistics.median(timings(fn, iters, repeats, warmup))


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


def head_row(B, H, W, dev, iters, repeats):
    Ci = 16
    g = torch.Generator().manual_seed(B + H)
    x, init = torch.randn((B, Ci, H, W), generator=g).to(dev), torch.randn((B, 1, H, W), generator=g).to(dev)
    w = (torch.randn((1, Ci, 3, 3), generator=g) / (9 * Ci) ** 0.5).to(dev)
    wp = ops.pack_conv2d_weights(w)
    fused = lambda: ops_deeppruner.refine_head_up2(x, w, init)                                             # noqa: E731
    composed = lambda: ops.bilinear_scale(ops.conv2d(x, wp, 1, 3, 1, 1, None, None, init, True), (2 * H, 2 * W), 2.0)   # noqa: E731
    res = dict(workload="refine_head", input=[B, Ci, H, W], max_abs_diff=(fused() - composed()).abs().max().item())
    t_f, t_c = timings(fused, iters, repeats), timings(composed, iters, repeats)
    res["fused_us"], res["composition_us"] = 1e3 * statistics.median(t_f), 1e3 * statistics.median(t_c)
    res["fused_spread_us"], res["composition_spread_us"] = 1e3 * (max(t_f) - min(t_f)), 1e3 * (max(t_c) - min(t_c))
    res["speedup"] = res["composition_us"] / res["fused_us"]
    must = 4 * B * H * W * (Ci + 1 + 4)
    res["fused_gbs"], res["composition_gbs"] = must / res["fused_us"] / 1e3, must / res["composition_us"] / 1e3
    res["fused_share_of_hbm_peak"] = res["fused_gbs"] / HBM_PEAK_GBS
    res["gate_met"] = res["composition_us"] - res["fused_us"] > res["composition_spread_us"]
    return res


def refinement_pair(planes, num, dev):
    stock = R.seeded_state(R.DeepPrunerRefinement(planes, True, num), 7).to(dev).eval()
    hip = DeepPrunerRefinement(list(planes), True, num)
    hip.load_state_dict(stock.state_dict(), strict=True)
    return hip.to(dev).eval(), stock


def refinement_inputs(planes, num, B, hw, dev):
    g = torch.Generator().manual_seed(B + hw[0])
    fms = [torch.randn((B, planes[i] - 1, hw[0] << i, hw[1] << i), generator=g).to(dev) for i in range(num)]
    return torch.randn((B, 1) + tuple(hw), generator=g).to(dev), fms


def refinement_row(tag, planes, num, B, hw, dev, iters, repeats):
    hip_m, stock_m = refinement_pair(planes, num, dev)
    disp, fms = refinement_inputs(planes, num, B, hw, dev)
    hip = lambda: hip_m([disp], fms)                                                                   # noqa: E731
    stock = lambda: stock_m([disp], fms)                                                               # noqa: E731
    a, b = hip(), stock()
    res = dict(workload="deeppruner_refinement", config=tag, in_planes_list=list(planes), first_stage=[B, planes[0] - 1] + list(hw),
               max_abs_diff=[(u - v).abs().max().item() for u, v in zip(a[:-1], b[:-1])], max_abs=[v.abs().max().item() for v in b[:-1]])
    del a, b
    res["hip_ms"] = timed(hip, iters, repeats)
    res["hip_graph_ms"] = timed(graphed(hip), iters, repeats)
    res["stock_ms"] = timed(stock, iters, repeats)
    res["speedup"], res["speedup_graph"] = res["stock_ms"] / res["hip_ms"], res["stock_ms"] / res["hip_graph_ms"]
    return res


def census(dev, iters, repeats):
    """Batch 1, the 4x config's stage: 2 copies + 6 fused convolutions + 1 fused head = 9 launches; per layer the HIP and the stock
    time on that layer's own input."""
    planes = [42]
    hip_m, stock_m = refinement_pair(planes, 1, dev)
    disp, fms = refinement_inputs(planes, 1, 1, HALF, dev)
    guide = torch.cat((fms[0], disp), 1)
    hb, sb = hip_m.refine_blocks[0], stock_m.refine_blocks[0]
    res = dict(workload="deeppruner_refinement_census", guide=list(guide.shape), launches=2 + 6 + 1, layers=[])
    res["guide_copies_us"] = 1e3 * timed(lambda: torch.cat((fms[0], disp), 1), iters, repeats)
    x = guide
    for i in range(6):
        u = hb.conv[i]
        row = dict(layer="conv.%d" % i, channels=[u.in_planes, u.out_planes], dilation=u.dilation)
        row["hip_us"] = 1e3 * timed(lambda: u(x), iters, repeats)
        row["stock_us"] = 1e3 * timed(lambda: sb.conv[i](x), iters, repeats)      # (its in-place ReLU acts on its own output)
        res["layers"].append(row)
        x = u(x)
    row = dict(layer="classify + add + relu + up2", channels=[16, 1])
    row["hip_us"] = 1e3 * timed(lambda: hb.classify(x, disp), iters, repeats)
    row["stock_us"] = 1e3 * timed(lambda: R.refine_tail(x, sb.classify.weight, disp), iters, repeats)
    res["layers"].append(row)
    return res


def backbone_row(name, cls, B, dev, iters, repeats):
    stock_m = R.seeded_state(getattr(R, cls.__name__)(3, True), 7).to(dev).eval()
    hip_m = cls()
    hip_m.load_state_dict(stock_m.state_dict(), strict=True)
    hip_m = hip_m.to(dev).eval()
    g = torch.Generator().manual_seed(B)
    left, right = torch.randn((B, 3, 544, 960), generator=g).to(dev), torch.randn((B, 3, 544, 960), generator=g).to(dev)
    hip = lambda: hip_m(left, right)                                                                   # noqa: E731
    stock = lambda: stock_m(left, right)                                                               # noqa: E731
    a, b = R.flatten(hip()[0]), R.flatten(stock()[0])
    res = dict(workload="deeppruner_backbone", backbone=name, images=[B, 3, 544, 960],
               max_abs_diff=[(u - v).abs().max().item() for u, v in zip(a, b)], max_abs=[v.abs().max().item() for v in b])
    del a, b
    res["hip_ms"] = timed(hip, iters, repeats)
    res["stock_ms"] = timed(stock, max(3, iters // 2), repeats)
    res["speedup"] = res["stock_ms"] / res["hip_ms"]
    return res


def stride2_row(k, B, dev, iters, repeats):
    g = torch.Generator().manual_seed(k + B)
    x = torch.randn((B, 64) + QUARTER, generator=g).to(dev)
    stock_u = R.seeded_state(R._conv_bn(True, 64, 128, k, 2, k // 2, 1, bias=False, relu=True), 9).to(dev).eval()
    hip_u = FusedConv2d(True, 64, 128, k, 2, k // 2, 1, bias=False, relu=True)
    hip_u.load_state_dict(stock_u.state_dict(), strict=True)
    hip_u = hip_u.to(dev).eval()
    half_u = FusedConv2d(True, 64, 64, k, 2, k // 2, 1, bias=False, relu=True).to(dev).eval()      # one launch of the kernel's widest stride-2 form
    res = dict(workload="stride2_64to128", kernel=k, input=list(x.shape), max_abs_diff=(hip_u(x) - stock_u(x)).abs().max().item())
    res["hip_two_launches_us"] = 1e3 * timed(lambda: hip_u(x), iters, repeats)
    res["hip_one_half_us"] = 1e3 * timed(lambda: half_u(x), iters, repeats)
    res["stock_us"] = 1e3 * timed(lambda: stock_u(x), iters, repeats)      # (in place on its own output only: the input is not touched)
    res["speedup"] = res["stock_us"] / res["hip_two_launches_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="head,refinement,census,backbone,stride2")
    args = ap.parse_args()
    only = set(args.only.split(","))
    dev = torch.device("cuda", 0)
    lines, failed = [], []

    def emit(res):
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

    with torch.no_grad():
        if "head" in only:
            for H, W in (HALF, QUARTER):
                for B in (1, 4):
                    row = head_row(B, H, W, dev, args.iters, args.repeats)
                    emit(row)
                    if not row["gate_met"]:
                        failed.append("refine_head %s" % row["input"])
        if "refinement" in only:
            for tag, planes, num, hw in (("4x", [42], 1, HALF), ("8x", [74, 33], 2, QUARTER)):
                for B in (1, 4):
                    row = refinement_row(tag, planes, num, B, hw, dev, args.iters, args.repeats)
                    emit(row)
                    if row["speedup"] <= 1.0 or row["speedup_graph"] <= 1.0:
                        failed.append("refinement %s batch %d" % (tag, B))
        if "census" in only:
            emit(census(dev, args.iters, args.repeats))
        if "backbone" in only:
            for name, cls in (("best", DeepPrunerBestBackbone), ("fast", DeepPrunerFastBackbone)):
                for B in (1, 4):
                    row = backbone_row(name, cls, B, dev, args.iters, args.repeats)
                    emit(row)
                    if row["speedup"] <= 1.0:
                        failed.append("backbone %s batch %d" % (name, B))
        if "stride2" in only:
            for k in (3, 1):
                for B in (1, 4):
                    emit(stride2_row(k, B, dev, args.iters, args.repeats))
    if args.out and lines:
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")
    if failed:
        sys.exit("a gate is not met at: " + "; ".join(failed))


if __name__ == "__main__":
    main()
