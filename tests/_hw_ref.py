"""Yardstick of the DeepPruner aggregator tests: ``HWHourglass`` and ``DeepPrunerAggregator`` restated in plain ``torch.nn`` with the
reference's ``state_dict`` keys (cost_processors/utils/hw_hourglass.py:27-105, aggregators/DeepPruner.py:23-59: Sequential(Conv3d |
ConvTranspose3d, BatchNorm3d[, ReLU]) units, bias-free).  Runs in FP32 and, after ``.double()``, in FP64, on any device.

``seeded_state(module, seed)`` fills ANY module with these keys (the restatement, the reference's modules, the HIP modules):
conv weights randn * sqrt(2 / fan_in) (fan_in = Ci * 27, for the stride-(1, 2, 2) transposed layers Ci * 27 / 4: a quarter of the
taps reach an output voxel on average), BatchNorm gamma and running_var in [0.5, 1.5], beta and running_mean in +-0.1.  Inputs and
weights of ``GOLDEN_CASES`` are regenerated from seeds, never stored; the reference's recorded outputs are in
tests/golden/deeppruner_aggregator.npz (scripts/gen_golden_deeppruner_aggregator.py)."""
import torch
import torch.nn as nn

HW = (1, 2, 2)


def _conv(bn, ci, co, stride=1, relu=True):
    layers = [nn.Conv3d(ci, co, 3, stride=stride, padding=1, bias=False)]
    if bn:
        layers.append(nn.BatchNorm3d(co))
    if relu:
        layers.append(nn.ReLU(inplace=True))
    return nn.Sequential(*layers)


def _deconv(bn, ci, co):
    layers = [nn.ConvTranspose3d(ci, co, 3, stride=HW, padding=1, output_padding=(0, 1, 1), bias=False)]
    if bn:
        layers.append(nn.BatchNorm3d(co))
    return nn.Sequential(*layers)


class HWHourglass(nn.Module):
    def __init__(self, in_planes, batch_norm=True):
        super().__init__()
        c = in_planes
        self.conv1_a, self.conv1_b, self.conv1_d = _conv(batch_norm, c, 2 * c, HW), _conv(batch_norm, 2 * c, 2 * c), _deconv(batch_norm, 2 * c, c)
        self.conv2_a, self.conv2_b, self.conv2_d = _conv(batch_norm, 2 * c, 4 * c, HW), _conv(batch_norm, 4 * c, 4 * c), _deconv(batch_norm, 4 * c, 2 * c)
        self.conv3_a, self.conv3_b, self.conv3_d = _conv(batch_norm, 4 * c, 8 * c, HW), _conv(batch_norm, 8 * c, 8 * c), _deconv(batch_norm, 8 * c, 4 * c)

    def forward(self, x):
        levels = []                                   # the output of each level on the way down
        for k in (1, 2, 3):
            down = getattr(self, "conv%d_a" % k)(x)
            x = getattr(self, "conv%d_b" % k)(down) + down
            levels.append(x)
        for k in (3, 2):                              # up again: each transposed layer meets the level above it
            x = getattr(self, "conv%d_d" % k)(x) + levels[k - 2]
        return self.conv1_d(x)


class DeepPrunerAggregator(nn.Module):
    def __init__(self, in_planes, hourglass_in_planes, batch_norm=True):
        super().__init__()
        hp = hourglass_in_planes
        self.dres0 = nn.Sequential(_conv(batch_norm, in_planes, 64), _conv(batch_norm, 64, 32))
        self.dres1 = nn.Sequential(_conv(batch_norm, 32, 32), _conv(batch_norm, 32, hp))
        self.dres2 = HWHourglass(hp, batch_norm)
        self.classify = nn.Sequential(_conv(batch_norm, hp, 2 * hp), nn.Conv3d(2 * hp, 1, 3, stride=1, padding=1, bias=False))

    def forward(self, volume):
        trunk = self.dres1(self.dres0(volume))
        return [self.classify(self.dres2(trunk) + trunk).squeeze(1)]


def seeded_state(module, seed):
    """Fill ``module`` in place, key by key in ``state_dict`` order from one seeded CPU generator; returns the module."""
    g = torch.Generator().manual_seed(seed)
    sd = module.state_dict()
    transposed = {name + ".weight" for name, m in module.named_modules() if isinstance(m, nn.ConvTranspose3d)}
    new = {}
    for key, t in sd.items():
        if key.endswith("num_batches_tracked"):
            v = torch.zeros(t.shape, dtype=t.dtype)
        elif t.dim() == 5:
            fan_in = t.shape[0] * 27 / 4.0 if key in transposed else t.shape[1] * 27
            v = torch.randn(t.shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif key.endswith("running_var") or key.endswith(".weight"):
            v = torch.rand(t.shape, generator=g) + 0.5
        else:                                                    # BatchNorm bias, running_mean
            v = torch.rand(t.shape, generator=g) * 0.2 - 0.1
        new[key] = v.to(dtype=t.dtype)
    module.load_state_dict(new)
    return module


IN_PLANES, HOURGLASS_IN_PLANES, WEIGHT_SEED = 21, 16, 1501
# name -> (input shape, input seed); "b": the deepest level is 1 x 5, "c": one disparity plane, taller than wide
GOLDEN_CASES = {"a": ((1, 21, 3, 16, 24), 11), "b": ((2, 21, 5, 8, 40), 12), "c": ((1, 21, 1, 24, 8), 13)}
# the hourglass alone (in_planes 16): recorded too
HOURGLASS_CASES = {"hg_a": ((1, 16, 2, 8, 8), 21), "hg_b": ((2, 16, 3, 16, 40), 22)}


def golden_input(name):
    shape, seed = (GOLDEN_CASES.get(name) or HOURGLASS_CASES[name])
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def aggregator(dtype=torch.float32):
    return seeded_state(DeepPrunerAggregator(IN_PLANES, HOURGLASS_IN_PLANES), WEIGHT_SEED).to(dtype).eval()


def hourglass(dtype=torch.float32):
    return seeded_state(HWHourglass(HOURGLASS_IN_PLANES), WEIGHT_SEED + 1).to(dtype).eval()


_fp64 = {}


def fp64_output(name):
    """FP64 evaluation of the restatement on the CPU for a golden case: computed once, shared, never modified."""
    if name not in _fp64:
        with torch.no_grad():
            if name in GOLDEN_CASES:
                out = aggregator(torch.float64)(golden_input(name).double())[0]
            else:
                out = hourglass(torch.float64)(golden_input(name).double())
        _fp64[name] = out
    return _fp64[name]
