"""The DeepPruner training losses on one GPU: the fused forward plus backward (csrc/deeppruner_loss.hip) against two baselines on
the SAME GPU.  One JSON line per size:

  (a) composition   the leanest composition of the library's existing kernels and elementwise torch, forward and backward written
                    out by hand (no autograd graph): per map one multiply, one division by a device scalar and one
                    ``ops.bilinear_scale``; two rescalings; ``ops.map_loss_fwd`` / ``map_loss_bwd`` per map; the quantile terms and
                    their derivative as masked elementwise torch (no boolean indexing, so no synchronisation);
                    ``ops.bilinear_scale_bwd`` and the tap scale per map.
  (b) stock         the plain torch restatement (tests/_deeppruner_loss_ref.py) under autograd, boolean indexing and its
                    synchronisations included.

Sizes: the training size [4, 1, 256, 512] and [1, 1, 544, 960], with both configs' maps (4x: list at 1/2 and 1/4, range maps at 1/4;
8x: list at 1/2, 1/4 and 1/8, range maps at 1/8).  Each figure is the median of ``--repeats`` HIP-event timings of ``--iters``
back-to-back calls, after a warm-up.  GB/s are on the bytes that must move: the low-resolution maps and gt once forward, the same
plus the gradients backward.  GATE: fused faster than (a) at every size by more than (a)'s own max - min spread.  Non-zero exit if
the gate fails.

    python scripts/bench_deeppruner_loss.py [--iters 10] [--repeats 5] [--out profiles/deeppruner_loss_bench.jsonl]
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
from tests import _deeppruner_loss_ref as R  # noqa: E402

HBM_PEAK_GBS = 8000.0                     # the MI355X's specified HBM3E peak
THETA, MAX_DISP = 0.05, 192.0
BOUNDS = (0.0, MAX_DISP, 0.0, MAX_DISP, THETA)
ROWS = [("4x", 4, 256, 512, 2), ("8x", 4, 256, 512, 3), ("4x", 1, 544, 960, 2), ("8x", 1, 544, 960, 3)]


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


def operands(B, H, W, K, dev):
    g = torch.Generator().manual_seed(B + K)
    coarse = torch.rand((B, 1, H // 16, W // 16), generator=g) * 300 - 45
    gt = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=True)
    gt = torch.where(torch.rand((B, 1, H, W), generator=g) < 0.03, torch.zeros(()), gt)

    def pooled(s, shift, spread):
        size = (H >> s, W >> s)
        return ((torch.nn.functional.adaptive_avg_pool2d(gt, size) + shift + spread * torch.randn((B, 1) + size, generator=g)) / (1 << s)).to(dev)
    return [pooled(k + 1, 0.0, 1.0) for k in range(K)], pooled(K, -1.0, 2.5), pooled(K, 1.0, 2.5), gt.to(dev)


def composition(disps, lo, hi, gt, go):
    """Forward and backward from the library's existing kernels; returns (K + 4 terms, gradients)."""
    dev, K, (H, W) = gt.device, len(disps), gt.shape[-2:]
    div = {n: torch.full((), float(n), device=dev) for n in {W} | {d.shape[-1] for d in disps + [lo]}}   # IEEE division on the device
    th = [torch.full((), THETA, device=dev), torch.full((), 1 - THETA, device=dev)]
    mask = ((gt > 0) & (gt < MAX_DISP)).float()
    nq = mask.sum()

    def run():
        ups = [ops.bilinear_scale((d * W) / div[d.shape[-1]], (H, W), 1.0) for d in disps + [lo, hi]]
        full = ups[:K] + [(ups[K] * W) / div[W], (ups[K + 1] * W) / div[W]]
        outs = [ops.map_loss_fwd(m, gt, 0.0, MAX_DISP, 1) for m in full]
        terms = [o[0] for o in outs]
        g_full = [ops.map_loss_bwd(m, gt, o, go[i:i + 1], 0.0, MAX_DISP, 1) for i, (m, o) in enumerate(zip(full, outs))]
        for j in range(2):
            x = gt - ups[K + j]
            below = (x < 0).float()
            terms.append((x * (th[j] - below) * mask).sum() / nq)
            g_full[K + j] = g_full[K + j] - (go[K + 2 + j] / nq) * mask * (th[j] - below)
        grads = [ops.bilinear_scale_bwd(g, tuple(d.shape[-2:]), 1.0) * (W / d.shape[-1]) for g, d in zip(g_full, disps + [lo, hi])]
        return torch.stack(terms), grads
    return run


def stock(disps, lo, hi, gt, coef):
    leaves = [t.detach().clone().requires_grad_() for t in disps + [lo, hi]]

    def run():
        for t in leaves:
            t.grad = None
        terms = R.terms(leaves[:-2], leaves[-2], leaves[-1], gt, THETA)
        sum(c * t for c, t in zip(coef, terms)).backward()
        return torch.stack([t.detach() for t in terms]), [t.grad for t in leaves]
    return run


def row(cfg, B, H, W, K, dev, iters, repeats):
    disps, lo, hi, gt = operands(B, H, W, K, dev)
    coef = R.coefficients(K + 4)
    go = torch.tensor(coef, dtype=torch.float32, device=dev)

    def fwd():
        return ops_deeppruner.deeppruner_loss_fwd(disps, lo, hi, gt, *BOUNDS)
    out, stats = fwd()

    def bwd():
        return ops_deeppruner.deeppruner_loss_bwd(disps, lo, hi, gt, stats, go, *BOUNDS)

    def fused():
        o, s = ops_deeppruner.deeppruner_loss_fwd(disps, lo, hi, gt, *BOUNDS)
        g_d, g_lo, g_hi = ops_deeppruner.deeppruner_loss_bwd(disps, lo, hi, gt, s, go, *BOUNDS)
        return o, g_d + [g_lo, g_hi]
    composed, plain = composition(disps, lo, hi, gt, go), stock(disps, lo, hi, gt, coef)
    res = dict(workload="deeppruner_loss", config=cfg, gt=[B, 1, H, W], K=K)
    (o_f, g_f), (o_c, g_c), (o_s, g_s) = fused(), composed(), plain()
    res["max_rel_diff_vs_composition"] = max([((o_f - o_c).abs() / o_c.abs()).max().item()]
                                             + [((a - b).abs().max() / b.abs().max()).item() for a, b in zip(g_f, g_c)])
    res["max_rel_diff_vs_stock"] = max([((o_f - o_s).abs() / o_s.abs()).max().item()]
                                       + [((a - b).abs().max() / b.abs().max()).item() for a, b in zip(g_f, g_s)])
    t = {n: timings(f, iters, repeats) for n, f in (("fused", fused), ("composition", composed), ("stock", plain), ("fused_fwd", fwd),
                                                    ("fused_bwd", bwd))}
    for n, ms in t.items():
        res[n + "_us"], res[n + "_spread_us"] = 1e3 * statistics.median(ms), 1e3 * (max(ms) - min(ms))
    maps = sum(d.numel() for d in disps + [lo, hi])
    must_f, must_b = 4 * (maps + gt.numel()), 4 * (2 * maps + gt.numel())
    res["must_move_mb_fwd"], res["must_move_mb_bwd"] = must_f / 1e6, must_b / 1e6
    res["fused_fwd_gbs"], res["fused_bwd_gbs"] = must_f / res["fused_fwd_us"] / 1e3, must_b / res["fused_bwd_us"] / 1e3
    res["fused_gbs"], res["composition_gbs"] = (must_f + must_b) / res["fused_us"] / 1e3, (must_f + must_b) / res["composition_us"] / 1e3
    res["fused_share_of_hbm_peak"] = res["fused_gbs"] / HBM_PEAK_GBS
    res["speedup_vs_composition"], res["speedup_vs_stock"] = res["composition_us"] / res["fused_us"], res["stock_us"] / res["fused_us"]
    res["gate_met"] = res["composition_us"] - res["fused_us"] > res["composition_spread_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deeppruner_loss.py needs a GPU: a timing from anything else says nothing")
    dev = torch.device("cuda:0")
    rows = [row(*r, dev, args.iters, args.repeats) for r in ROWS]
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")
    if not all(r["gate_met"] for r in rows):
        raise SystemExit("gate failed: the fused losses are not faster than the composition by more than its spread")


if __name__ == "__main__":
    main()
