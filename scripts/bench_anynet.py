"""AnyNet eval forward on one GPU: the HIP path against stock PyTorch-ROCm (tests/_anynet_ref.py, i.e. MIOpen convolutions and
ATen elementwise kernels, with this project's SPN op standing in for the restatement's Python loop) on the SAME GPU.  For each
size prints one JSON line: ms per pair at batch 1 (eager, and the HIP path through GraphedForward), pairs/s at batch 8, and
launches per forward.  The restatement moves its linspace samples from the host on every call (as the reference does,
cost_processors/AnyNet.py:61-62), so it cannot be captured into a graph; it runs eagerly.

    python scripts/bench_anynet.py [--sizes 544x960,384x1248] [--iters 50]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from densematchingbenchmark_amd import ops  # noqa: E402
from densematchingbenchmark_amd.config import Config  # noqa: E402
from densematchingbenchmark_amd.graph_runner import GraphedForward  # noqa: E402
from densematchingbenchmark_amd.modeling import build_model  # noqa: E402
from tests import _anynet_ref as R  # noqa: E402
from tests.test_anynet_host import golden_state  # noqa: E402


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="544x960,384x1248")
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "AnyNet", "scene_flow.py"))
    sd = golden_state()
    model = build_model(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval().requires_grad_(False)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    pcfg = cfg.model.cost_processor
    spn = lambda X, G1, G2, G3: ops.spn_gaterecurrent2d(X, G1, G2, G3, True, False)   # noqa: E731
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        res = dict(workload="anynet_eval", size=[H, W])
        with torch.no_grad():
            for B in (1, 8):
                left, right = (t.to(dev) for t in R.golden_inputs((B, 3, H, W), 5))
                batch = dict(leftImage=left, rightImage=right)
                hip = lambda: model(batch)                                       # noqa: E731
                stock = lambda: R.forward(left, right, sd_dev, pcfg, spn=spn)    # noqa: E731
                if B == 1:
                    res["hip_eager_ms"] = timed(hip, args.iters)
                    runner = GraphedForward(model)
                    res["hip_graph_ms"] = timed(lambda: runner(batch), args.iters)
                    res["hip_launches"] = launches(hip)
                    res["stock_eager_ms"] = timed(stock, args.iters)
                    res["stock_launches"] = launches(stock)
                else:
                    res["hip_b8_pairs_per_s"] = 8 * 1000.0 / timed(hip, max(5, args.iters // 4))
                    res["stock_b8_pairs_per_s"] = 8 * 1000.0 / timed(stock, max(5, args.iters // 4))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
