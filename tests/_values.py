"""Value distributions for the conditioning tests, named once.

A distribution fills one channel of a [B, C, *spatial] tensor, ``[B, S]`` values; ``mixed`` deals the named distributions
round-robin over the channels so that one launch of a per-channel kernel sees several of them.  Everything is FP32, finite and
deterministic per seed (one torch.Generator per channel, seeded by (seed, channel))."""
import functools

import torch

SIGMA = 1.5      # of ``plain`` and of everything derived from it
MU = 0.3


def _randn(B, S, gen):
    return torch.randn((B, S), generator=gen)


def _plain(B, S, gen):
    return _randn(B, S, gen) * SIGMA + MU


def _offset(k):
    def f(B, S, gen):        # mean = k sigma
        return _randn(B, S, gen) * SIGMA + k * SIGMA
    return f


def _outlier(k):
    def f(B, S, gen):        # the channel's first element (the pivot of the batch-statistics kernel) k sigma away from the rest
        v = _plain(B, S, gen)
        v[0, 0] += k * SIGMA
        return v
    return f


DISTRIBUTIONS = {
    "plain": _plain,                                                              # what the rest of the suite draws
    "offset100": _offset(100.0),
    "offset1000": _offset(1000.0),
    "tiny": lambda B, S, gen: _randn(B, S, gen) * 0.01 + 50.0,                    # |mean| / std = 5000
    "constant": lambda B, S, gen: torch.full((B, S), 3.0),
    "outlier30": _outlier(30.0),
    "outlier100": _outlier(100.0),
    "outlier1000": _outlier(1000.0),
    "sparse": lambda B, S, gen: torch.relu(_randn(B, S, gen) - 1.3),              # ~90 % zeros: a post-ReLU map
    "scaled_up": lambda B, S, gen: _plain(B, S, gen) * 1e4,
    "scaled_down": lambda B, S, gen: _plain(B, S, gen) * 1e-3,
}
NAMES = tuple(DISTRIBUTIONS)


def channel(name, B, S, seed):
    """[B, S] float32 values of distribution ``name``."""
    gen = torch.Generator().manual_seed(int(seed))
    return DISTRIBUTIONS[name](B, S, gen).to(torch.float32)


def channel_names(C, names=NAMES, first=0):
    """The distribution of each of C channels: ``names`` round-robin, starting at names[first]."""
    return [names[(first + ch) % len(names)] for ch in range(C)]


def mixed(shape, seed, names=NAMES, first=0):
    """A [B, C, *spatial] float32 tensor whose channel ch follows channel_names(C, names, first)[ch]; returns (tensor, names)."""
    B, C = int(shape[0]), int(shape[1])
    S = 1
    for d in shape[2:]:
        S *= int(d)
    per = channel_names(C, names, first)
    t = torch.stack([channel(per[ch], B, S, seed * 1000 + ch) for ch in range(C)], dim=1)
    return t.reshape(shape).contiguous(), per


def centre_tap_conv_inputs(shape, Co, offset, seed, w_scale=0.1):
    """Operands of a 3x3x3, padding-1 convolution whose raw output is a random part plus exactly ``offset`` in every output channel:
    ``shape`` = (B, Ci, D, H, W) with the LAST input channel constant 1 and weight ``offset`` on its centre tap only (the centre tap
    is in range at every voxel, borders included), zero on its other 26 taps.  Returns (x, w)."""
    B, Ci, D, H, W = shape
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randn(shape, generator=g)
    w = torch.randn((Co, Ci, 3, 3, 3), generator=g) * w_scale
    x[:, Ci - 1] = 1.0
    w[:, Ci - 1] = 0.0
    w[:, Ci - 1, 1, 1, 1] = float(offset)
    return x, w


# ---------------------------------------------------------------------------------------------- the tolerance rule
# |kernel - FP64| <= 4 x |FP32 reference - FP64| + 2e-6 x (range): ``close`` over a whole output, ``check_per_channel`` PER CHANNEL --
# every channel is judged against its own FP32-reference error and its own range, so a well-conditioned channel cannot lend its
# range (or a badly conditioned one its reference error) to another.
FLOOR = 2e-6


def close(got, ref64, ref32, what, floor=FLOOR):
    """|got - FP64| must stay within 4x the FP32 oracle's own error (plus a floor, default 2e-6, of the value range)."""
    scale = ref64.abs().max().item()
    err = (got.double() - ref64).abs().max().item()
    own = (ref32.double() - ref64).abs().max().item()
    assert err <= 4 * own + floor * scale, "%s: error %.3e vs oracle FP32 error %.3e (range %.3e)" % (what, err, own, scale)


def per_channel_max(t, C):
    """max |t| over everything but the channel axis: [C] stays, [B, C, ...] -> [C]."""
    t = t.abs().double()
    if t.dim() == 1:
        return t
    return t.transpose(0, 1).reshape(C, -1).max(dim=1).values


def check_per_channel(got, ref64, ref32, what, names, scale=None, cap=False):
    """Rule of the conditioning tests for one output.  ``scale``: the [C] range the floor is relative to (default: the channel's
    largest |FP64 value|).  ``cap``: also hold 1e-6 * max(1, |value|) + 2e-7 where that is the tighter bound (the bound
    test_batch_statistics_from_the_convolution_epilogue already puts on scale / shift / the running buffers)."""
    C = len(names)
    got, ref32 = got.detach().cpu(), ref32.detach().cpu()
    assert torch.isfinite(got).all(), what
    err = per_channel_max(got.double() - ref64, C)
    own = per_channel_max(ref32.double() - ref64, C)            # (``ref32``: the yardstick, FP32 or built on FP32-stored values)
    rng = per_channel_max(ref64, C)
    bound = 4 * own + FLOOR * (rng if scale is None else scale.double())
    if cap:
        bound = torch.minimum(bound, 1e-6 * rng.clamp(min=1.0) + 2e-7)
    lines = ["%-14s %-12s err %.3e  FP32 reference %.3e  bound %.3e  range %.3e%s" %
             (what, names[ch], err[ch], own[ch], bound[ch], rng[ch], "   <-- outside" if err[ch] > bound[ch] else "") for ch in range(C)]
    print("\n".join(lines))
    bad = [l for ch, l in enumerate(lines) if not err[ch] <= bound[ch]]
    assert not bad, "\n" + "\n".join(bad)


def bn_forward_reference(c, gamma, beta, rm0, rv0, momentum=0.1, eps=1e-5):
    """Training-mode BatchNorm of ``c`` ([B, C, *spatial], CPU FP32) without activation: dicts (FP64, FP32) of mean, invstd, scale,
    shift, running_mean, running_var, y, and the [C] FP64 standard deviation.  FP64: plain torch.  FP32: ATen's batch_norm."""
    C = c.shape[1]
    dims = [0] + list(range(2, c.dim()))
    view = [1, C] + [1] * (c.dim() - 2)
    n = c.numel() // C
    c64, g64, b64 = c.double(), gamma.double(), beta.double()
    mean = c64.mean(dim=dims)
    var = ((c64 - mean.view(view)) ** 2).mean(dim=dims)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = g64 * invstd
    shift = b64 - mean * scale
    r64 = dict(mean=mean, invstd=invstd, scale=scale, shift=shift,
               running_mean=rm0.double() + momentum * (mean - rm0.double()),
               running_var=rv0.double() + momentum * (var * n / max(n - 1, 1) - rv0.double()),
               y=(c64 - mean.view(view)) * scale.view(view) + b64.view(view))
    rm, rv = rm0.clone(), rv0.clone()
    y32, m32, i32 = torch.native_batch_norm(c, gamma, beta, rm, rv, True, momentum, eps)
    s32 = gamma * i32
    h32 = beta - m32 * s32
    r32 = dict(mean=m32, invstd=i32, scale=s32, shift=h32, running_mean=rm, running_var=rv, y=y32,
               y_stored=c * s32.view(view) + h32.view(view))
    return r64, r32, torch.sqrt(var)


def bn_backward_reference(c, gamma, beta, dy, eps=1e-5):
    """Backward of training-mode BatchNorm without activation: dicts of dc, dgamma, dbeta -- (FP64, ATen's FP32 autograd, stored).
    ``stored`` is FP64 arithmetic on ATen's FP32 mean and invstd: the backward reads the statistics as the FP32 vectors the forward
    wrote (the unit's ABI), so xhat = (c - mean) * invstd carries the rounding of ``mean``, |mean| * 2^-24 / std -- 1e-4 for ``tiny``
    -- and dgamma = sum dy * xhat that bias times dbeta, whatever the summation does.  ATen's FP32 autograd has the same bias AND
    its own FP32 accumulation on top; ``stored`` has the bias alone, so 4x its error is the tighter yardstick."""
    from oracle import dmb_oracle as O
    r32 = O.bn_act_train(c, gamma, beta, None, 0, eps=eps, dy=dy)
    r64 = O.bn_act_train(c, gamma, beta, None, 0, eps=eps, dy=dy, dtype=torch.float64)
    C = c.shape[1]
    dims = [0] + list(range(2, c.dim()))
    view = [1, C] + [1] * (c.dim() - 2)
    n = c.numel() // C
    _, m32, i32 = torch.native_batch_norm(c, gamma, beta, None, None, True, 0.1, eps)
    xhat = (c.double() - m32.double().view(view)) * i32.double().view(view)
    dbeta = dy.double().sum(dim=dims)
    dgamma = (dy.double() * xhat).sum(dim=dims)
    dc = (gamma.double() * i32.double()).view(view) * (dy.double() - dbeta.view(view) / n - xhat * dgamma.view(view) / n)
    keys = ("dc", "dgamma", "dbeta")
    return {k: r64[k] for k in keys}, {k: r32[k] for k in keys}, dict(dc=dc, dgamma=dgamma, dbeta=dbeta)


# ``offset1000`` and ``tiny`` (|mean| / std of 1000 and 5000).  The unit's ABI hands the normalisation on as an FP32 (scale, shift)
# pair -- to dmb_bn_act_f32, to the convolution epilogues, and bn_train_fwd must equal bn_train_stats + bn_act bit for bit -- and
# y = c * scale + shift then carries the rounding of shift = beta - mean * scale, half a unit in the last place of |mean| / std:
# 6e-5 at 1000, 2.4e-4 for ``tiny``.  ATen's y does not (it is (c - mean) * invstd * gamma + beta there: measured 4e-7 and 1e-5 on
# these channels where the kernel has 6e-5 and 1.3e-4).  So for these two distributions, and for y alone, the FP32 yardstick is the
# FP32 evaluation of c * scale + shift with ATen's statistics: what any holder of the FP32 pair can compute.  The bound is still 4x
# that reference's measured error plus the floor.  ``offset100`` and ``constant`` meet ATen's y as it is and are judged by it, and
# mean, invstd, scale, shift and the running buffers of every channel are judged against ATen.
STORAGE_BOUND_Y = ("offset1000", "tiny")


def check_bn_forward(got, c, gamma, beta, rm0, rv0, names, momentum=0.1, stored_y=None):
    """``got``: dict of the kernel's mean, invstd, scale, shift, running_mean, running_var, y for the CPU FP32 tensor ``c``.
    ``stored_y``: per channel, whether y is judged by the stored (scale, shift) form (default: names in STORAGE_BOUND_Y)."""
    r64, r32, std = bn_forward_reference(c, gamma, beta, rm0, rv0, momentum)
    # the mean relative to the spread it is subtracted from, or to its own FP32 spacing where the channel has none
    mean_scale = torch.maximum(std, r64["mean"].abs() * 2.0 ** -23)
    check_per_channel(got["mean"], r64["mean"], r32["mean"], "mean", names, scale=mean_scale)
    check_per_channel(got["invstd"], r64["invstd"], r32["invstd"], "invstd", names)
    check_per_channel(got["scale"], r64["scale"], r32["scale"], "scale", names, cap=True)
    check_per_channel(got["shift"], r64["shift"], r32["shift"], "shift", names, cap=True)
    # running_mean = rm0 + momentum * (mean - rm0) in FP32: its rounding follows the larger of the two operands
    rm_scale = torch.maximum(torch.maximum(r64["running_mean"].abs(), rm0.double().abs()), momentum * mean_scale)
    check_per_channel(got["running_mean"], r64["running_mean"], r32["running_mean"], "running_mean", names, scale=rm_scale)
    check_per_channel(got["running_var"], r64["running_var"], r32["running_var"], "running_var", names, cap=True)
    if stored_y is None:
        stored_y = [n in STORAGE_BOUND_Y for n in names]
    pick = torch.tensor(stored_y).view([1, len(names)] + [1] * (c.dim() - 2))
    check_per_channel(got["y"], r64["y"], torch.where(pick, r32["y_stored"], r32["y"]), "y", names)


# ---------------------------------------------------------------------------------------------- the cases
# The smallest shapes that reach every path of norm.hip's for_slice: four slices of float4; 64 slices with several float4 per
# lane; S % 4 != 0 (the dword path); a 3-D unit.  Each shape is run once per group of its channel count, so that every shape sees
# every distribution.
SHAPES = ((2, 4, 4096), (2, 2, 65536), (2, 3, 33, 31), (3, 8, 5, 6, 12))
CASES = tuple((shape, first) for shape in SHAPES for first in range(0, len(NAMES), shape[1]))


def case_id(case):
    shape, first = case
    return "%s-%s" % ("x".join(str(d) for d in shape), "+".join(channel_names(shape[1], first=first)))


def _vec(C, seed, scale=1.0, offset=0.0):
    return torch.randn((C,), generator=torch.Generator().manual_seed(seed)) * scale + offset


@functools.lru_cache(maxsize=None)
def bn_case(shape, first):
    """Operands of one conditioning case (CPU FP32; shared between tests, never written to)."""
    C = shape[1]
    c, names = mixed(shape, 7, first=first)
    dy = torch.randn(shape, generator=torch.Generator().manual_seed(11 + first))
    return dict(c=c, names=names, dy=dy, gamma=_vec(C, 2, 0.5, 1.0), beta=_vec(C, 3, 0.2), rm0=_vec(C, 6, 0.1), rv0=_vec(C, 7).abs() + 0.5)


EPILOGUE_SHAPES = ((2, 16, 6, 7, 24), (1, 32, 5, 9, 32))      # (B, Ci, D, H, W) of the input; 32 output channels
EPILOGUE_OFFSETS = (0.0, 200.0, 2000.0)                          # |mean| / std of the raw output about 0, 100 and 1000
