"""Yardstick of the DeepPruner aggregator BACKWARD tests: forward + backward of the restatement of tests/_hw_ref.py (plain torch.nn,
any dtype) on seeded weights and inputs, with a fixed random projection of the output as the loss.  Shared by the host test, the GPU
test and scripts/gen_golden_deeppruner_aggregator_bwd.py, which records the REAL reference's results in
tests/golden/deeppruner_aggregator_bwd.npz after asserting that this restatement equals them bit for bit on the CPU.

A RUN is (case, mode): mode "eval" = eval() with trainable weights (running statistics, buffers untouched), "train" = train()
(batch statistics, buffers updated) -- only at the first shape of each pair, which keeps >= 60 values per channel at the deepest
level (hourglass 2 x 3 x 2 x 5, aggregator 2 x 4 x 2 x 4 = 64).

The golden file holds, per run ``<case>/<mode>/``: ``loss``; ``dx`` (the input gradient in full -- for agg_a/train, which would
take the file past the repository's 1 MiB limit, ``dx_stats`` and ``dx_samples`` instead: sum, largest magnitude, SAMPLES_DX entries
at seeded positions); per parameter ``p/<name>/stats`` (sum, largest magnitude) and ``p/<name>/samples`` (SAMPLES entries at seeded
positions, all of a smaller tensor); in train mode the updated running buffers ``b/<name>``."""
import zlib

import torch

from tests import _hw_ref as R

# name -> (kind, input shape, input seed)
CASES = {
    "hg_a": ("hourglass", (2, 16, 3, 16, 40), 31),
    "hg_b": ("hourglass", (1, 16, 2, 8, 8), 32),
    "agg_a": ("aggregator", (2, 21, 4, 16, 32), 33),
    "agg_b": ("aggregator", (1, 21, 2, 8, 24), 34),
}
RUNS = [("hg_a", "eval"), ("hg_a", "train"), ("hg_b", "eval"), ("agg_a", "eval"), ("agg_a", "train"), ("agg_b", "eval")]
SAMPLES, SAMPLES_DX = 64, 4096
SAMPLED_DX = {("agg_a", "train")}
# compared tensors: the input, every convolution weight, every gamma and beta
N_TENSORS = {"hourglass": 1 + 9 + 2 * 9, "aggregator": 1 + (4 + 9 + 2) + 2 * (4 + 9 + 1)}


def case_input(name):
    _, shape, seed = CASES[name]
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def projection(name, shape):
    """The fixed random tensor whose inner product with the output is the loss"""
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(CASES[name][2] + 500))


def fill(module, name):
    """Seeded weights for any module with the reference's keys (restatement, reference, HIP module)"""
    return R.seeded_state(module, R.WEIGHT_SEED + (1 if CASES[name][0] == "hourglass" else 0))


def restatement(name, mode, dtype=torch.float32):
    kind = CASES[name][0]
    m = R.HWHourglass(R.HOURGLASS_IN_PLANES) if kind == "hourglass" else R.DeepPrunerAggregator(R.IN_PLANES, R.HOURGLASS_IN_PLANES)
    return fill(m, name).to(dtype).train(mode == "train")


def positions(key, numel, n=SAMPLES):
    """Seeded flat positions into a tensor of ``numel`` entries (all of them when it has no more than ``n``)"""
    if numel <= n:
        return torch.arange(numel)
    return torch.randint(numel, (n,), generator=torch.Generator().manual_seed(zlib.crc32(key.encode()) & 0x7fffffff))


def run(module, name, forward=None, device="cpu", dtype=torch.float32):
    """Forward + backward of ``module`` on the case's input -> dict(out, loss, dx, grads {parameter: gradient}, buffers).
    ``forward(module, x)``: default the module's own call; an aggregator's one-element list is unwrapped."""
    x = case_input(name).to(device=device, dtype=dtype).requires_grad_()
    for p in module.parameters():
        p.grad = None
    out = forward(module, x) if forward is not None else module(x)
    if isinstance(out, (list, tuple)):
        (out,) = out
    loss = (out * projection(name, out.shape).to(device=device, dtype=dtype)).sum()
    loss.backward()
    return dict(out=out.detach(), loss=loss.detach(), dx=x.grad, grads={k: p.grad for k, p in module.named_parameters()},
                buffers={k: v.detach().clone() for k, v in module.named_buffers()})


_cache = {}


def reference(name, mode, dtype):
    """The restatement's run on the CPU in ``dtype``: computed once, shared, never modified."""
    key = (name, mode, dtype)
    if key not in _cache:
        _cache[key] = run(restatement(name, mode, dtype), name, dtype=dtype)
    return _cache[key]


def whole_network_rule(got, ref64, ref32, what):
    """The rule of tests/test_backward_gpu.py for gradients through a whole network, where a ReLU may flip: every tensor within 3e-2
    of its range, at least 60 % of them within 4 |fp32 - fp64| + 2e-5 x range.  ``got`` / ``ref64`` / ``ref32``: {name: tensor}.
    -> (tensors compared, tensors within the tight bound)"""
    tight = 0
    assert sorted(got) == sorted(ref64), (what, sorted(set(got) ^ set(ref64)))
    for k, r64 in ref64.items():
        assert got[k] is not None, (what, k)
        g, r64, r32 = got[k].detach().cpu().double(), r64.detach().double(), ref32[k].detach().double()
        scale = r64.abs().max().item()
        err = (g - r64).abs().max().item()
        assert err <= 3e-2 * scale, "%s: grad of %s: error %.3e of range %.3e" % (what, k, err, scale)
        tight += err <= 4 * (r32 - r64).abs().max().item() + 2e-5 * scale
    assert tight >= 0.6 * len(ref64), "%s: only %d of %d gradients within the tight tolerance" % (what, tight, len(ref64))
    return len(ref64), tight


def tensors(res):
    """{name: tensor} of a run's compared gradients: the input's and every parameter's"""
    d = {"input": res["dx"]}
    d.update(res["grads"])
    return d
