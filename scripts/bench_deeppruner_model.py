"""The DeepPruner model on one GPU: the fused output tail (csrc/deeppruner_final_maps.hip) against the composition it replaces, and
the whole eval forward against stock PyTorch-ROCm running the plain ``torch.nn`` restatement (tests/_deeppruner_model_ref.py) with
the same weights on the SAME GPU.  One JSON line per measurement:

  final_maps               ``ops_deeppruner.deeppruner_final_maps`` against the composition it replaces, at its leanest: per map
                           one multiply, one division by a device scalar made beforehand and one ``ops.bilinear_scale`` (K + 2
                           maps), two rescalings of two launches, two subtractions and two ``abs`` -- 3 (K + 2) + 8 launches --
                           at [1|4] x 544 x 960 for K = 2 (range maps at 1/4) and K = 3 (at 1/8); GB/s on the bytes that must move
                           and the composition's own run-to-run spread (max - min of its repeats).
                           GATE: faster at every row by more than that spread.
  deeppruner_model         both configs, batch 1 and 4 -- HIP eager, HIP replayed from a captured graph, stock -- with PatchMatch's
                           noise in the batch, and the stock / HIP ratios.  4x at 544 x 960 and 384 x 1248; 8x, whose images must be
                           multiples of 64 (features at 1/8 under hourglasses of three stride-2 levels), at 576 x 960 (its
                           config's evaluation size) and 384 x 1280.                      GATE: HIP faster at every row, both ways.
  deeppruner_model_census  batch 1 at the first size: device kernels of one forward by the profiler's count, the library's own
                           apart from torch's copies.

Each figure is the median of ``--repeats`` HIP-event timings of ``--iters`` back-to-back calls, after a warm-up.  Non-zero exit if a
gate fails.

    python scripts/bench_deeppruner_model.py [--iters 10] [--repeats 5] [--out profiles/deeppruner_model_bench.jsonl]
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
from densematchingbenchmark_amd.config import Config  # noqa: E402
from densematchingbenchmark_amd.modeling.stereo.models import DeepPruner  # noqa: E402
from tests import _deeppruner_model_ref as R  # noqa: E402

HBM_PEAK_GBS = 8000.0                     # the MI355X's specified HBM3E peak
SIZES = {"4x": ((544, 960), (384, 1248)), "8x": ((576, 960), (384, 1280))}


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


def tail_row(B, H, W, K, dev, iters, repeats):
    g = torch.Generator().manual_seed(B + K)
    disps = [(torch.rand((B, 1, H >> k, W >> k), generator=g) * 50).to(dev) for k in range(K)]
    lo = (torch.rand((B, 1, H >> K, W >> K), generator=g) * 30).to(dev)
    hi = lo + 10
    fused = lambda: ops_deeppruner.deeppruner_final_maps(disps, lo, hi, (H, W))                          # noqa: E731
    div = {n: torch.full((), float(n), device=dev) for n in {W} | {d.shape[-1] for d in disps + [lo]}}   # IEEE division on the device

    def composed():
        ups = [ops.bilinear_scale((d * W) / div[d.shape[-1]], (H, W), 1.0) for d in disps + [lo, hi]]
        D, Mn, Mx = ups[K - 1], ups[K], ups[K + 1]
        return ups[:K] + [(Mn * W) / div[W], (Mx * W) / div[W], torch.abs(D - Mn), torch.abs(Mx - D)]
    res = dict(workload="final_maps", output=[K + 4, B, 1, H, W], K=K, composition_launches=3 * (K + 2) + 8,
               bit_identical=all(torch.equal(a, b) for a, b in zip(fused(), composed())))
    t_f, t_c = timings(fused, iters, repeats), timings(composed, iters, repeats)
    res["fused_us"], res["composition_us"] = 1e3 * statistics.median(t_f), 1e3 * statistics.median(t_c)
    res["fused_spread_us"], res["composition_spread_us"] = 1e3 * (max(t_f) - min(t_f)), 1e3 * (max(t_c) - min(t_c))
    res["speedup"] = res["composition_us"] / res["fused_us"]
    must = 4 * B * (sum((H >> k) * (W >> k) for k in range(K)) + 2 * (H >> K) * (W >> K) + (K + 4) * H * W)
    res["must_move_mb"] = must / 1e6
    res["fused_gbs"], res["composition_gbs"] = must / res["fused_us"] / 1e3, must / res["composition_us"] / 1e3
    res["fused_share_of_hbm_peak"] = res["fused_gbs"] / HBM_PEAK_GBS
    res["gate_met"] = res["composition_us"] - res["fused_us"] > res["composition_spread_us"]
    return res


def model_pair(name, dev):
    stock = R.model(name).to(dev)
    hip = DeepPruner(Config.fromfile(os.path.join(ROOT, R.CASES[name][0])))
    hip.load_state_dict(stock.state_dict(), strict=True)
    return hip.to(dev).eval(), stock


def model_inputs(name, B, hw, dev):
    g = torch.Generator().manual_seed(B + hw[0])
    s = 2 << len(R.CASES[name][3])
    left = torch.randn((B, 3) + tuple(hw), generator=g)
    right = torch.roll(left, -6, dims=3) + 0.1 * torch.randn((B, 3) + tuple(hw), generator=g)
    noise = torch.rand((B, R.PATCH_MATCH_SAMPLES - 2, hw[0] // s, hw[1] // s), generator=g)
    return left.to(dev), right.to(dev), noise.to(dev)


def model_row(name, B, hw, dev, iters, repeats):
    hip_m, stock_m = model_pair(name, dev)
    left, right, noise = model_inputs(name, B, hw, dev)
    batch = dict(leftImage=left, rightImage=right, patchMatchNoise=noise)
    hip = lambda: hip_m(batch)[0]["disps"]                                                               # noqa: E731
    stock = lambda: stock_m(left, right, noise)["disps"]                                                 # noqa: E731
    a, b = hip(), stock()
    res = dict(workload="deeppruner_model", config=name, images=[B, 3] + list(hw),
               max_abs_diff=[(u - v).abs().max().item() for u, v in zip(a, b)], max_abs=[v.abs().max().item() for v in b])
    del a, b
    res["hip_ms"] = timed(hip, iters, repeats)
    res["hip_graph_ms"] = timed(graphed(hip), iters, repeats)
    res["stock_ms"] = timed(stock, max(3, iters // 2), repeats)
    res["speedup"], res["speedup_graph"] = res["stock_ms"] / res["hip_ms"], res["stock_ms"] / res["hip_graph_ms"]
    return res


def census(name, dev):
    from torch.profiler import ProfilerActivity, profile
    hip_m, _ = model_pair(name, dev)
    hw = SIZES[name][0]
    left, right, noise = model_inputs(name, 1, hw, dev)
    batch = dict(leftImage=left, rightImage=right, patchMatchNoise=noise)
    hip_m(batch)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        hip_m(batch)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]
    own = [n for n in kernels if "dmb" in n]
    counts = {}
    for n in kernels:
        if "dmb" not in n:
            counts[n[:60]] = counts.get(n[:60], 0) + 1
    return dict(workload="deeppruner_model_census", config=name, images=[1, 3] + list(hw), kernels=len(kernels), library=len(own),
                final_maps=len([n for n in own if "deeppruner_final_maps" in n]), memcpy=len(names) - len(kernels), torch_kernels=counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="tail,model,census")
    args = ap.parse_args()
    only = set(args.only.split(","))
    dev = torch.device("cuda", 0)
    lines, failed = [], []

    def emit(res):
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        if args.out:                       # written as the run goes: a run that is cut short keeps what it measured
            with open(args.out, "w") as fp:
                fp.write("\n".join(lines) + "\n")

    with torch.no_grad():
        if "tail" in only:
            for K in (2, 3):
                for B in (1, 4):
                    row = tail_row(B, 544, 960, K, dev, args.iters, args.repeats)
                    emit(row)
                    if not row["gate_met"]:
                        failed.append("final_maps %s" % row["output"])
        if "model" in only:
            for name in R.CASES:
                for hw in SIZES[name]:
                    for B in (1, 4):
                        row = model_row(name, B, hw, dev, args.iters, args.repeats)
                        emit(row)
                        if row["speedup"] <= 1.0 or row["speedup_graph"] <= 1.0:
                            failed.append("model %s %s batch %d" % (name, hw, B))
        if "census" in only:
            for name in R.CASES:
                emit(census(name, dev))
    if failed:
        sys.exit("a gate is not met at: " + "; ".join(failed))


if __name__ == "__main__":
    main()
