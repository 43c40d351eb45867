"""Development aid: A/B the whole PSMNet step (bench.py's configuration) under development options, alternating the variants
inside ONE process on ONE chip (numbers from different gpurun boxes differ by ~1 %).
    python scripts/ab_step.py "4=1" "10=2" "4=1,10=2"      each argument: comma-separated option=value pairs of a variant"""
import os, sys
os.environ.setdefault("DMB_LIB", "dev")   # kernel-variant switches exist only in the development build (build.py --dev)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from densematchingbenchmark_amd import _lib, ops, ops_head, synthetic
from densematchingbenchmark_amd.config import Config
from densematchingbenchmark_amd.modeling import build_model

dev = torch.device("cuda:0")
lib = _lib.load()
cfg = Config.fromfile(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", *os.environ.get("AB_CONFIG", "PSMNet/scene_flow.py").split("/")))
model = build_model(cfg, backbone=None).eval()
synthetic.init_params_(model, seed=0, classif_gain=10.0)
model = model.to(dev)
_Hp, _Wp = cfg.data.eval.input_shape
left, right = synthetic.feature_batch(0, 1, 4, 32, _Hp // 4, _Wp // 4, dev)
batch = dict(leftFeature=left, rightFeature=right)
# an option is "<development option index>=<value>", or "fls=0" (first-layer convolutions on one stream), "ovl=1" (branch overlap),
# "hd=0" (classifier branches as two launches instead of the fused head; needs no development build: run with DMB_LIB= )
def _parse(kv):
    k, v = kv.split("=")
    return (k if k in ("fls", "ovl", "hd") else int(k), int(v))


_head_applicable = ops_head.conv3d_k3_head_applicable


def _set(k, v):
    if k == "fls":     # 2 = merged launch (default), 1 = three streams, 0 = serial
        ops.set_first_layer_mode({2: "merged", 1: "streams", 0: "serial"}[v])
    elif k == "ovl":
        ops.set_branch_overlap(bool(v))
    elif k == "hd":
        ops_head.conv3d_k3_head_applicable = _head_applicable if v else (lambda x: False)
    else:
        lib.dmb_dev_set_option(k, v)


_DEFAULT = {"fls": 2, "ovl": 0, "hd": 1}
variants = [("default", [])] + [(a, [_parse(kv) for kv in a.split(",")]) for a in sys.argv[1:]]


def run(n):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        model(batch)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


with torch.no_grad():
    run(5)
    acc = {name: [] for name, _ in variants}
    for rep in range(4):
        for name, opts in variants:
            for k, v in opts:
                _set(k, v)
            run(2)
            acc[name].append(run(8))
            for k, _ in opts:
                _set(k, _DEFAULT.get(k, 0))
print("# whole PSMNet step (batch 4, %dx%d, D = 192) under development options, variants alternated in one process on one chip (4 x 8 steps each);" % (_Hp, _Wp))
print("# 13=1: narrow stride-1 planes on box tiles instead of 64-voxel runs; 4=1: deconv3d_kernel (round-2 transposed convolution) instead of "
      "deconv3d_zy_kernel; 16=R: zy item order in groups of R tiles; 20=1: ONE class-major zy item list (round-3 order); 10=2: stride-2 four-row tiles "
      "with the dword epilogue; 19=k: stride-1 tile candidate k - 1; fls=0 / 1: first-layer convolutions as five launches on one stream / on three streams; ovl=1: branch overlap; "
      "hd=0: classifier branches as 32 -> 32 + 32 -> 1 launches instead of the fused head")
for name, ts in acc.items():
    print("%-24s %s  -> min %.3f ms, median %.3f ms" % (name, " ".join("%.3f" % t for t in ts), min(ts), sorted(ts)[len(ts) // 2]))
