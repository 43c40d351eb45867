"""Autograd of the cost-path units on the HIP kernels (second part).

What torch.autograd does for the reference's ``nn.Sequential(Conv3d | ConvTranspose3d, BatchNorm3d[, ReLU])`` units
(dmb/modeling/stereo/layers/basic_layers.py:68-100,160-177), its skip adds (cost_processors/utils/hourglass.py:62-86),
the cost-volume builders (cost_processors/utils/cat_fms.py:7-48, dif_fms.py:7-46) and the up-sampling + soft-argmin
tail (aggregators/PSMNet.py:74-93, disp_predictors/faster_soft_argmin.py:51-75), expressed as ``autograd.Function``s
whose forward and backward are HIP kernel launches:

  forward   raw = conv(x, w) (+ bias)              the inference kernel without its epilogue
            y = act(raw*scale + shift (+ skip)) with scale/shift from
              batch statistics (a BatchNorm in training mode; running buffers updated)     bn_train_fwd
              the running buffers (a BatchNorm in eval mode), or 1 / 0 (no BatchNorm)       bn_act
  backward  dc, dgamma, dbeta, dskip <- dy                                                  bn_act_bwd
            dw = wgrad(x, dc)                                                               conv3d_k3[s2]_wgrad
            dx = the forward kernel of the adjoint convolution on re-packed weights         conv3d_k3 / deconv3d_k3s2

There is no fallback to torch's convolution backward: without the library these raise like every other op.
"""
import contextlib
import threading
import weakref

import torch

from .... import ops, ops_deeppruner, param_state

_RELU = {0: False, 1: True, 2: "pre"}
_CONST = {}

# ---------------------------------------------------------------------------------------------- gradient carry (round 6)
# A tensor with several consumers (the skip operands of hourglass.py:62-86 and PSMNet.py:58-72: cost0 has four, pre1 three)
# gets its gradient as a SUM over them, and torch.autograd forms that sum with one addition launch per extra consumer -- three
# passes over a 200 MB tensor each, 18 of them per PSMNet step (0.75 ms of 31).  Inside a ``carry_scope()`` every unit hands
# the tensors it consumes on as identity outputs ("aliases": the same storage, a new autograd edge) and the NEXT consumer of the
# tensor is quietly given the alias instead.  The consumers then form a chain, each one's backward receives what the later
# consumers have already collected, and adds its own share inside a kernel that runs anyway: the data-gradient convolution
# takes it as its skip operand (one extra read), the BatchNorm backward as ``dres_acc``.  Same gradients up to the order of
# the FP32 additions; ``set_gradient_carry(False)`` switches it off (tests/test_train_gpu.py compares the two).
_carry_enabled = True
_tls = threading.local()      # the open scope's registry belongs to the thread that runs the forward pass


def set_gradient_carry(flag):
    global _carry_enabled
    _carry_enabled = bool(flag)


def _registry():
    return getattr(_tls, "registry", None)


@contextlib.contextmanager
def carry_scope():
    """One forward pass of a model / aggregator.  The registry maps id(tensor) -> (tensor, its latest alias) and lives exactly as
    long as the scope (a tensor object the caller re-uses across steps must never meet an alias of an earlier graph); nested
    scopes share the outermost registry; one registry per thread."""
    if _registry() is not None:
        yield
        return
    _tls.registry = {}
    try:
        yield
    finally:
        _tls.registry.clear()
        _tls.registry = None


def _latest(reg, t):
    while True:
        e = reg.get(id(t))
        if e is None:
            return t
        t = e[1]


def _carry_plan(x, skip):
    """(registry or None, x, skip, carry_x, carry_skip) for a unit about to consume x (and skip)."""
    reg = _registry()
    if reg is None or not _carry_enabled or not torch.is_grad_enabled():
        return None, x, skip, False, False
    x = _latest(reg, x)
    if skip is not None:
        skip = _latest(reg, skip)
    cx = x.requires_grad and x.is_contiguous() and x.dtype == torch.float32
    cs = skip is not None and skip is not x and skip.requires_grad and skip.is_contiguous() and skip.dtype == torch.float32
    return reg, x, skip, cx, cs


def _const(value, C, device):
    """Cached [C] tensor of ones / zeros (identity scale / shift of units without BatchNorm): no fill launch per call."""
    key = (float(value), int(C), str(device))
    t = _CONST.get(key)
    if t is None:
        t = _CONST[key] = torch.full((C,), float(value), dtype=torch.float32, device=device)
    return t


def _relu_code(relu):
    return 2 if relu == "pre" else (1 if relu else 0)


def _mask_mode(code, has_skip):
    """Which tensor the backward takes the ReLU mask from.  Without a skip operand ``y = max(fma(raw, scale, shift), 0)``, so
    ``y > 0`` IS ``fma(raw, scale, shift) > 0`` bit for bit: the backward passes re-create the mask from ``raw`` (which they read
    anyway) and the unit's output is neither read again nor kept alive for it -- one tensor less in each of the two passes for
    16 of PSMNet's 25 units."""
    return _RELU[2 if code == 1 and not has_skip else code]


class _PackGroup:
    """Packed weights of every 3-D unit that has taken the training path on one device: the forward AND the data-gradient pack of
    all of them are re-made by ONE launch (ops.run_pack_table) instead of one launch per unit and direction (52 launches of 4.8 us
    in a PSMNet step).  The pack buffers and the device table of pack jobs persist; units are held weakly.

    Re-packed, all units at once, when the asking unit's weight no longer matches its stamp (param_state): an in-place update, or
    an optimizer step, which advances the epoch -- one launch per training step.  Code that writes parameters where ``_version``
    cannot see it (``.data`` in-place writes, raw pointers) calls ``bump_param_epoch()``.  Before every launch, units that died
    or whose weight moved leave the group and the table of raw pointers is rebuilt: a dead or moved job is never launched."""

    def __init__(self, device):
        self.device, self.entries, self.table, self.njobs = device, {}, None, 0

    def packs(self, unit, weight):
        e = self.entries.get(id(unit))
        if e is None or e["unit"]() is not unit or not e["stamp"].holds((weight,)):
            if e is None or e["unit"]() is not unit or not e["stamp"].placed((weight,)):
                jobs = ops.unit_pack_jobs(weight, unit.transposed, unit.stride)
                e = {"unit": weakref.ref(unit), "stamp": param_state.Stamp((weight,)), "jobs": jobs,
                     "bufs": [torch.empty((ops.packed_floats(co, ci),), dtype=torch.float32, device=weight.device)
                              for co, ci, _ in jobs]}
                self.entries[id(unit)] = e
                self.table = None
            self._repack()
        return e["bufs"]

    def _repack(self):
        weights = {k: u[0].weight for k, u in ((k, e["unit"]()) for k, e in self.entries.items()) if u is not None}
        live = {k: e for k, e in self.entries.items() if k in weights and e["stamp"].placed((weights[k],))}
        if self.table is None or len(live) != len(self.entries):
            jobs = [(weights[k].detach(), buf, co, ci, mode)
                    for k, e in live.items() for (co, ci, mode), buf in zip(e["jobs"], e["bufs"])]
            self.entries, self.table, self.njobs = live, ops.make_pack_table(jobs, self.device), len(jobs)
        ops.run_pack_table(self.table, self.njobs)
        for k, e in self.entries.items():
            e["stamp"] = param_state.Stamp((weights[k],))


_pack_groups = {}
_pack_group_enabled = True


def set_pack_group(flag):
    """False: one pack launch per unit, direction and call, as in rounds 1-5 (A/B and tests; the 2-D units' phase packs too)."""
    global _pack_group_enabled
    _pack_group_enabled = bool(flag)


def _unit_packs(unit, w):
    """(forward pack, data-gradient pack) of a unit's weight; the data-gradient pack may be None (made on demand)."""
    weight = unit[0].weight
    if not _pack_group_enabled or torch.cuda.is_current_stream_capturing() or not weight.is_contiguous():
        fwd = ops.pack_deconv3d_weights(w) if unit.transposed else ops.pack_conv3d_weights(w)
        return fwd, None
    key = (w.device.type, w.device.index)
    g = _pack_groups.get(key)
    if g is None:
        g = _pack_groups[key] = _PackGroup(w.device)
    return tuple(g.packs(unit, weight))


def _bias_as_shift(bias):
    """(scale, shift) operands that make a convolution kernel add the unit's bias in its epilogue; (None, None) without one."""
    if bias is None:
        return None, None
    return _const(1.0, bias.numel(), bias.device), bias.detach().contiguous()


def _conv_raw(unit, x, wpack, bias):
    """The unit's convolution without BatchNorm / activation (+ bias through the kernel's shift operand)."""
    Co = unit.out_planes
    scale, shift = _bias_as_shift(bias)
    if unit.transposed:
        if unit.stride == unit.HW:
            return ops.deconv3d_k3s2(x, wpack, Co, scale, shift, None, False, stride=unit.HW)
        return ops.deconv3d_k3s2(x, wpack, Co, scale, shift, None, False)
    return ops.conv3d_k3(x, wpack, Co, scale, shift, None, unit.stride, False)


# Batch statistics out of the convolution's epilogue (conv3d_s1_kernel's STATS instantiation + ops.bn_train_act; VERDICT round 5,
# "not attempted" twice).  Built, tested -- and OFF by default, because it does not pay: at 4 x 256x512 the six units it covers lose
# their 33 us statistics pass each (-0.20 ms) but the convolution's epilogue grows by 16 us (+0.10 ms: the FP64 sums, the lane
# butterfly and a barrier sit in the one part of that kernel nothing overlaps) and the normalising pass, which now finishes 3072
# partials per channel instead of 128, by 8 us (+0.05 ms): 27.2 ms per step either way (docs/design/12-6).
_epilogue_stats = False


def set_epilogue_stats(flag):
    """True: 32-channel stride-1 units take the block sums of their batch statistics from the convolution's epilogue."""
    global _epilogue_stats
    _epilogue_stats = bool(flag)


def _batch_stats(bn):
    """nn.BatchNorm's rule: batch statistics in training mode, and always for a BatchNorm that keeps no running buffers
    (``track_running_stats=False``), whatever its mode."""
    return bn is not None and (bn.training or bn.running_mean is None or bn.running_var is None)


def _bn_momentum(bn):
    """The factor of nn.BatchNorm's running-buffer update: ``momentum``, or with ``momentum=None`` the cumulative moving
    average's 1 / (batches seen including this one) -- 0 for a BatchNorm that keeps no running buffers."""
    if bn.momentum is not None:
        return bn.momentum
    return 1.0 / float(int(bn.num_batches_tracked) + 1) if bn.track_running_stats else 0.0


def _running_affine(bn, gamma, beta, C, device):
    """(mean, invstd, scale, shift) of a BatchNorm that normalises with its running buffers and leaves them alone -- eval mode,
    also inside a model in train() (fine-tuning with frozen statistics) -- or the cached identity of a unit without BatchNorm."""
    if bn is None:
        zero, one = _const(0.0, C, device), _const(1.0, C, device)
        return zero, one, one, zero
    mean = bn.running_mean.detach().float()
    invstd = torch.rsqrt(bn.running_var.detach().float() + bn.eps)
    scale = (gamma.detach() if gamma is not None else torch.ones_like(mean)) * invstd
    shift = (beta.detach() if beta is not None else torch.zeros_like(mean)) - mean * scale
    return mean, invstd, scale, shift


def _unit_bn_forward(bn, raw, gamma, beta, skip, code, C, device, partials=None):
    """BatchNorm (+ skip, + ReLU) of a unit's raw convolution output -> (y, mean, invstd, scale, shift, batch_stats).  A
    batch-statistics BatchNorm takes the two-launch form (ops.bn_train_fwd: block sums, then one kernel that finishes the
    statistics, updates the running buffers and the batch counter and normalises); running statistics / no BatchNorm: bn_act."""
    if _batch_stats(bn):
        momentum = _bn_momentum(bn)     # (read before the batch counter below moves)
        nbt = bn.num_batches_tracked if bn.track_running_stats and bn.num_batches_tracked is not None else None
        if nbt is not None and nbt.device != raw.device:
            nbt += 1
            nbt = None
        args = (gamma.detach() if gamma is not None else None, beta.detach() if beta is not None else None,
                bn.running_mean if bn.track_running_stats else None, bn.running_var if bn.track_running_stats else None, nbt, momentum,
                bn.eps, skip, _RELU[code])
        if partials is not None:   # the convolution's epilogue already summed its output: no pass for the block sums
            y, mean, invstd, scale, shift = ops.bn_train_act(raw, partials, *args)
        else:
            y, mean, invstd, scale, shift = ops.bn_train_fwd(raw, *args)
        return y, mean, invstd, scale, shift, True
    mean, invstd, scale, shift = _running_affine(bn, gamma, beta, C, device)
    y = raw if (bn is None and skip is None and code == 0) else ops.bn_act(raw, scale, shift, skip, _RELU[code])
    return y, mean, invstd, scale, shift, False


# ---------------------------------------------------------------------------------------------- the unit skeleton
# ConvUnitFn (3-D) and Conv2dUnitFn (2-D) are one function of (x, weight, bias, gamma, beta, skip, unit, relu, carry_x, carry_skip)
# around a different convolution: each holds its forward launch and its choice of gradient launches, the rest is here.
def _unit_params(unit):
    """(conv, bn or None, gamma, beta) of a Fused unit; gamma / beta are None without an affine BatchNorm."""
    bn = unit[1] if unit.has_bn else None
    affine = bn is not None and bn.affine
    return unit[0], bn, (bn.weight if affine else None), (bn.bias if affine else None)


def _apply_carried(fn, unit, x, residual, relu):
    """``fn`` (ConvUnitFn | Conv2dUnitFn) on the unit's parameters; inside a carry scope x and the skip operand are replaced
    by their latest aliases and the aliases this call returns are registered for their next consumer."""
    conv, _, gamma, beta = _unit_params(unit)
    reg, x, residual, cx, cs = _carry_plan(x, residual)
    out = fn.apply(x, conv.weight, conv.bias, gamma, beta, residual, unit, relu, cx, cs)
    if not (cx or cs):
        return out
    for t, alias in zip(((x,) if cx else ()) + ((residual,) if cs else ()), out[1:]):
        reg[id(t)] = (t, alias)
    return out[0]


def _unit_forward_tail(ctx, unit, raw, x, w, x_in, gamma, beta, bias, skip, relu, carry_x, carry_skip, partials=None):
    """BatchNorm / activation of the raw convolution output, everything the backward pass needs on ``ctx``, and the outputs:
    y alone, or (y, x_in, skip) with the inputs handed on as identity outputs (gradient carry, top of this file)."""
    code = _relu_code(relu)
    y, mean, invstd, scale, shift, batch_stats = _unit_bn_forward(_unit_params(unit)[1], raw, gamma, beta, skip, code, unit.out_planes,
                                                                  x.device, partials)
    ctx.unit, ctx.code, ctx.batch_stats = unit, code, batch_stats
    ctx.has = (bias is not None, gamma is not None, beta is not None, skip is not None)
    ctx.carry = (bool(carry_x), bool(carry_skip))
    ctx.save_for_backward(x, w, raw, y if code == 1 and skip is not None else None, scale, shift, mean, invstd)
    if not (carry_x or carry_skip):
        return y
    ctx.set_materialize_grads(False)   # an alias nobody consumed has no gradient: None, not a tensor of zeros
    return (y,) + ((x_in,) if carry_x else ()) + ((skip,) if carry_skip else ())


def _unit_backward_head(ctx, grads):
    """The BatchNorm / activation backward -> (dc, what x's later consumers collected or None, the saved x and w, and
    bn_grads = (dgamma, dbeta, dres, need_dres, scale) for _unit_backward_tail)."""
    g = list(grads)
    dy = g.pop(0)
    dx_acc = g.pop(0) if ctx.carry[0] else None
    dres_acc = g.pop(0) if ctx.carry[1] else None    # what skip's later consumers collected
    x, w, raw, y, scale, shift, mean, invstd = ctx.saved_tensors
    code, has_skip = ctx.code, ctx.has[3]
    dy = torch.zeros_like(raw) if dy is None else dy.contiguous()
    need_dres = has_skip and ctx.needs_input_grad[5]
    if not need_dres:
        dres_acc = None
    dc, dgamma, dbeta, dres = ops.bn_act_bwd(dy, raw, y, scale, shift, mean, invstd, _mask_mode(code, has_skip), ctx.batch_stats,
                                             want_dres=need_dres and code == 1, dres_acc=dres_acc)
    if need_dres and code != 1 and dres_acc is None:
        dres = dy                       # the skip branch joins after the activation (or there is none)
    return dc, dx_acc, x, w, (dgamma, dbeta, dres, need_dres, scale)


def _unit_dbias(batch_stats, scale, dbeta):
    """The bias gradient, the sum of dc over (batch, voxels), without another pass: dc = scale * (dpre - mean terms), so it is
    dbeta times scale with running statistics (or no BatchNorm: scale = 1) and exactly zero behind batch statistics (sum xhat = 0:
    the normalisation removes any constant the bias adds)."""
    return torch.zeros_like(dbeta) if batch_stats else scale * dbeta


def _affine_grads(ctx, has_gamma, has_beta, at, dgamma, dbeta):
    """(dgamma, dbeta) as backward returns them for inputs ``at``, ``at + 1``: None for one that was None or wants no gradient."""
    needs = ctx.needs_input_grad
    return dgamma if has_gamma and needs[at] else None, dbeta if has_beta and needs[at + 1] else None


def _unit_backward_tail(ctx, dx, dw, bn_grads):
    dgamma, dbeta, dres, need_dres, scale = bn_grads
    has_bias, has_gamma, has_beta, _ = ctx.has
    dbias = _unit_dbias(ctx.batch_stats, scale, dbeta) if has_bias and ctx.needs_input_grad[2] else None
    return (dx, dw, dbias) + _affine_grads(ctx, has_gamma, has_beta, 3, dgamma, dbeta) + (dres if need_dres else None, None, None, None, None)


class ConvUnitFn(torch.autograd.Function):
    """y = act(BN(conv(x)) (+ skip)) of one FusedConv3d unit; ``unit`` supplies the geometry and the BN buffers.  With
    ``carry_x`` / ``carry_skip`` the inputs are handed on as identity outputs (gradient carry, top of this file)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, skip, unit, relu, carry_x=False, carry_skip=False):
        x_in = x
        x = x.contiguous()
        w = weight.detach().contiguous()
        wp_fwd, wp_bwd = _unit_packs(unit, w)
        C = unit.out_planes
        bn = _unit_params(unit)[1]
        partials = None
        if (_epilogue_stats and _batch_stats(bn) and bias is None and not unit.transposed and unit.stride == 1 and C == 32):
            # the statistics' block sums come out of the convolution's own epilogue (32-channel stride-1 units: 6 of PSMNet's 25)
            fused = ops.conv3d_k3_bnstats(x, wp_fwd, C)
            if fused is not None:
                raw, partials = fused
        if partials is None:
            raw = _conv_raw(unit, x, wp_fwd, bias)
        # (the data-gradient pack belongs to the weight version of THIS forward: autograd forbids changing the weight before the
        # backward pass, and the group only re-packs when a version moved)
        ctx.wp_bwd, ctx.w_version = wp_bwd, weight._version
        return _unit_forward_tail(ctx, unit, raw, x, w, x_in, gamma, beta, bias, skip, relu, carry_x, carry_skip, partials)

    @staticmethod
    def backward(ctx, *grads):
        dc, dx_acc, x, w, bn_grads = _unit_backward_head(ctx, grads)
        unit = ctx.unit
        dw = dx = None
        if ctx.needs_input_grad[1]:
            if unit.transposed:
                dw = ops.deconv3d_k3s2_wgrad(x, dc)
            elif unit.stride in (2, unit.HW):     # (the library reads which of the two from the operands' depths)
                dw = ops.conv3d_k3s2_wgrad(x, dc)
            else:
                dw = ops.conv3d_k3_wgrad(x, dc)
        if ctx.needs_input_grad[0]:
            wp = ctx.wp_bwd if w._version == ctx.w_version else None
            dx = (ops.deconv3d_k3s2_dgrad(dc, w, residual=dx_acc, wpack=wp, stride=unit.stride) if unit.transposed
                  else ops.conv3d_k3_dgrad(dc, w, unit.stride, tuple(x.shape[2:]), residual=dx_acc, wpack=wp))
        return _unit_backward_tail(ctx, dx, dw, bn_grads)


def conv_unit(unit, x, residual=None, relu=False):
    """Differentiable forward of a FusedConv3d unit (``relu``: False / True = after the skip add / 'pre' = before it)."""
    return _apply_carried(ConvUnitFn, unit, x, residual, relu)


class CatConvUnitFn(torch.autograd.Function):
    """The aggregator's FIRST unit on a concatenation / difference volume of unit disparity step (aggregators/PSMNet.py:31-35 on
    cat_fms.py:7-48, aggregators/StereoNet.py on dif_fms.py:7-46) without the volume in the forward pass: the convolution runs
    in its 2-D form on the two feature maps (csrc/catconv.hip, as the eval path does since round 2 -- a third of the layer's
    multiplications, no 400 MB volume written and read), BatchNorm / ReLU as in ConvUnitFn.  The backward pass does not build the
    volume either: the weight gradient folds z of dc into 2 x 9 maps per channel and is two 2-D weight gradients against them
    (ops.cat_first_wgrad); the data gradient -- only when the feature maps want one -- is the 3-D convolution it is, folded onto
    the maps with the builders' adjoint.  A PSMNet training step at 4 x 256x512: forward of the first unit 1.24 -> 0.2 ms, its
    weight gradient 1.28 -> 0.2 ms."""

    @staticmethod
    def forward(ctx, left, right, weight, bias, gamma, beta, unit, relu, disp_idx, kind):
        left, right = left.contiguous(), right.contiguous()
        w = weight.detach().contiguous()
        sc, sh = _bias_as_shift(bias)
        raw = ops.catconv_first(left, right, len(disp_idx), ops.catconv_pack(w, kind), sc, sh, False)
        code = _relu_code(relu)
        y, mean, invstd, scale, shift, batch_stats = _unit_bn_forward(_unit_params(unit)[1], raw, gamma, beta, None, code,
                                                                      unit.out_planes, left.device)
        ctx.unit, ctx.code, ctx.batch_stats, ctx.disp_idx, ctx.kind = unit, code, batch_stats, tuple(disp_idx), kind
        ctx.has = (bias is not None, gamma is not None, beta is not None)
        ctx.save_for_backward(left, right, w, raw, scale, shift, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        left, right, w, raw, scale, shift, mean, invstd = ctx.saved_tensors
        has_bias, has_gamma, has_beta = ctx.has
        idx = list(ctx.disp_idx)
        dc, dgamma, dbeta, _ = ops.bn_act_bwd(dy.contiguous(), raw, None, scale, shift, mean, invstd, _mask_mode(ctx.code, False),
                                              ctx.batch_stats)
        dw = dL = dR = dbias = None
        if ctx.needs_input_grad[2]:
            if left.shape[-1] % 4 == 0:
                dw = ops.cat_first_wgrad(left, right, dc, ctx.kind)      # z folded into 2-D maps: no volume here either
            else:
                vol = ops.cat_fms(left, right, idx) if ctx.kind == "cat" else ops.dif_fms(left, right, idx)
                dw = ops.conv3d_k3_wgrad(vol, dc)
                del vol
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dvol = ops.conv3d_k3_dgrad(dc, w, 1)
            dL, dR = ops.cat_fms_bwd(dvol, idx) if ctx.kind == "cat" else ops.dif_fms_bwd(dvol, idx)
        if has_bias and ctx.needs_input_grad[3]:
            dbias = _unit_dbias(ctx.batch_stats, scale, dbeta)
        return ((dL if ctx.needs_input_grad[0] else None, dR if ctx.needs_input_grad[1] else None, dw, dbias)
                + _affine_grads(ctx, has_gamma, has_beta, 4, dgamma, dbeta) + (None, None, None, None))


def cat_conv_unit(unit, lazy, relu=False):
    """Differentiable forward of a FusedConv3d unit on a LazyCatVolume (the caller has checked ops.catconv_applicable)."""
    conv, _, gamma, beta = _unit_params(unit)
    return CatConvUnitFn.apply(lazy.reference_fm, lazy.target_fm, conv.weight, conv.bias, gamma, beta, unit, relu,
                               tuple(lazy.disp_idx), lazy.kind)


class HeadConvFn(torch.autograd.Function):
    """nn.Conv3d(C, 1, 3, 1, 1) (+ bias) (+ the cumulative cost add of PSMNet.py:71-72)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual):
        x = x.contiguous()
        w = weight.detach().contiguous()
        ctx.save_for_backward(x, w)
        ctx.has = (bias is not None, residual is not None)
        y = ops.conv3d_k3_c1(x, w, 0.0, residual)
        # the kernel takes its bias as a host scalar; reading the parameter back every step would stall the stream, so the
        # 1-channel result gets it from the device tensor
        return y + bias.detach().view(1, 1, 1, 1, 1) if bias is not None else y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = dbias = None
        if ctx.needs_input_grad[0]:
            dx = ops.conv3d_k3_dgrad(dy, w, 1)              # a convolution 1 -> C on the mirrored taps
        if ctx.needs_input_grad[1]:
            dw = ops.conv3d_k3_wgrad(x, dy)
        if ctx.has[0] and ctx.needs_input_grad[2]:
            dbias = dy.sum().reshape(1)
        return dx, dw, dbias, (dy if ctx.has[1] and ctx.needs_input_grad[3] else None)


class HeadDeconvFn(torch.autograd.Function):
    """nn.ConvTranspose3d(C, Co <= 32, 3, stride 2, padding 1, output_padding 1, bias) without BatchNorm / activation: GC-Net's
    output layer (aggregators/GCNet.py:63-67)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        w = weight.detach().contiguous()
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return ops.deconv3d_k3s2(x, ops.pack_deconv3d_weights(w), w.shape[1], None,
                                 bias.detach().float().contiguous() if bias is not None else None, None, False)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        return (ops.deconv3d_k3s2_dgrad(dy, w) if ctx.needs_input_grad[0] else None,
                ops.deconv3d_k3s2_wgrad(x, dy) if ctx.needs_input_grad[1] else None,
                dy.sum(dim=(0, 2, 3, 4)) if ctx.has_bias and ctx.needs_input_grad[2] else None)


class CatFmsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, left, right, disp_idx):
        ctx.disp_idx = tuple(disp_idx)
        return ops.cat_fms(left, right, list(disp_idx))

    @staticmethod
    def backward(ctx, dvol):
        dL, dR = ops.cat_fms_bwd(dvol.contiguous(), list(ctx.disp_idx))
        return dL, dR, None


class DifFmsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, left, right, disp_idx):
        ctx.disp_idx = tuple(disp_idx)
        return ops.dif_fms(left, right, list(disp_idx))

    @staticmethod
    def backward(ctx, dvol):
        dL, dR = ops.dif_fms_bwd(dvol.contiguous(), list(ctx.disp_idx))
        return dL, dR, None


FAST_FMS_BWD_MAX_W = 1024   # dmb_fast_fms_bwd_f32: 2 * 8 channels * W * 4 bytes of LDS <= 64 KiB


def fast_samples_for_autograd(disp_sample, like):
    """The samples as FastFmsFn takes them (FP32, contiguous, on the features' device) without cutting their autograd history."""
    if disp_sample.requires_grad and torch.is_grad_enabled() and disp_sample.dim() != 4:
        raise NotImplementedError("fast_cat_fms / fast_dif_fms: a gradient for the samples needs per-pixel samples [B, D, H, W]")
    return disp_sample.float().to(like.device).contiguous()


class FastFmsFn(torch.autograd.Function):
    """fast_cat_fms / fast_dif_fms under autograd (csrc/warp_volume.hip): gradients for the two feature maps (the sampler's
    adjoint) and, when they require one, for per-pixel disparity samples (the sampler's column derivative: the route AnyNet's
    and DeepPruner's predicted disparities take, AnyNet.py:60-73, DeepPruner.py:192).  ``normalize`` = fast_dif_fms's p-norm
    over the channels (dif_fms.py:82-84)."""

    @staticmethod
    def forward(ctx, left, right, disp_sample, dif, normalize=False, p=1.0):
        if left.shape[-1] > FAST_FMS_BWD_MAX_W:   # refuse here, not inside backward(): the adjoint keeps 2 x 8 rows of W floats in LDS
            raise NotImplementedError("fast_cat_fms / fast_dif_fms under autograd: feature maps wider than %d columns have no "
                                      "backward on the HIP path (the forward alone has no such limit: run it under torch.no_grad())"
                                      % FAST_FMS_BWD_MAX_W)
        if normalize and not dif:
            raise ValueError("normalize belongs to fast_dif_fms")
        ctx.dif, ctx.p = bool(dif), float(p)
        out = ops.fast_dif_fms(left, right, disp_sample, normalize, p) if dif else ops.fast_cat_fms(left, right, disp_sample)
        ctx.save_for_backward(left, right, disp_sample, out if normalize else None)
        return out

    @staticmethod
    def backward(ctx, dvol):
        left, right, disp_sample, norm_out = ctx.saved_tensors
        dL, dR, dS = ops.fast_fms_bwd(left, right, disp_sample, dvol.contiguous(), ctx.dif, norm_out, ctx.p,
                                      wrt_samples=ctx.needs_input_grad[2])
        return dL, dR, dS, None, None, None


class UpsampleRegressFn(torch.autograd.Function):
    """(cost [B, Do, Ho, Wo], disp [B, 1, Ho, Wo]) of a low-resolution cost [B, Di, Hi, Wi].  Differentiable through the
    disparity (the path every PSMNet loss takes, without the full-size gradient volume) and through the volume itself."""

    @staticmethod
    def forward(ctx, x, size, values, alpha):
        x = x.contiguous()
        cost, disp = ops.trilinear_ac_soft_argmin(x, size, values, alpha)
        ctx.save_for_backward(x, disp)
        ctx.size, ctx.values, ctx.alpha = tuple(size), tuple(values), float(alpha)
        ctx.set_materialize_grads(False)
        return cost, disp

    @staticmethod
    def backward(ctx, dcost, ddisp):
        if dcost is None and ddisp is None:
            return None, None, None, None
        x, disp = ctx.saved_tensors
        if ddisp is None:   # only a loss on the volume
            return ops.trilinear_ac_bwd(dcost.contiguous(), tuple(x.shape[1:])), None, None, None
        return ops.trilinear_ac_soft_argmin_bwd(x, disp, ddisp.contiguous(), ctx.size, list(ctx.values), ctx.alpha,
                                                grad_cost=dcost.contiguous() if dcost is not None else None), None, None, None


class DeconvK8S4Fn(torch.autograd.Function):
    """AcfNet's learned up-sampling nn.ConvTranspose3d(1, 1, 8, 4, 2) on a squeezed cost [B, D, H, W] (AcfNet.py:55-57,81-83)."""

    @staticmethod
    def forward(ctx, x, weight):
        x = x.contiguous()
        w = weight.detach().contiguous().view(8, 8, 8)
        ctx.save_for_backward(x, w)
        ctx.wshape = tuple(weight.shape)
        return ops.deconv3d_k8s4_c1(x, w)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx, dw = ops.deconv3d_k8s4_c1_bwd(x, w, dy.contiguous(), ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dx, (dw.view(ctx.wshape) if dw is not None else None)


class ConfHeadFn(torch.autograd.Function):
    """Confidence logits of one AcfNet head (cmn/cmn.py:21-36): Conv2d(D -> D/3, 3x3) + BatchNorm2d + ReLU + Conv2d(-> 1, 1x1),
    no biases.  Forward and backward are 2-D launches of the same kernel families as the 3-D units."""

    @staticmethod
    def forward(ctx, cost, w1, gamma, beta, w2, head):
        cost = cost.contiguous()
        w1d, w2d = w1.detach().contiguous(), w2.detach().contiguous()
        Cm = w1d.shape[0]
        raw = ops.conv2d(cost, ops.pack_conv2d_weights(w1d), Cm, 3)
        bn = head.conf_net[0][1] if head.batch_norm else None
        h, mean, invstd, scale, shift, batch_stats = _unit_bn_forward(bn, raw, gamma, beta, None, 1, Cm, cost.device)
        logit = ops.conv2d(h, ops.pack_conv2d_weights(w2d), 1, 1)
        ctx.batch_stats = batch_stats
        ctx.has = (gamma is not None, beta is not None)
        ctx.save_for_backward(cost, w1d, w2d, raw, h, scale, shift, mean, invstd)
        return logit

    @staticmethod
    def backward(ctx, dlogit):
        cost, w1, w2, raw, h, scale, shift, mean, invstd = ctx.saved_tensors
        dlogit = dlogit.contiguous()
        dh = ops.conv2d_dgrad(dlogit, w2)                                  # 1 -> Cm channels
        dw2 = ops.channel_dot(h, dlogit).view_as(w2) if ctx.needs_input_grad[4] else None
        dc, dgamma, dbeta, _ = ops.bn_act_bwd(dh, raw, None, scale, shift, mean, invstd, "pre", ctx.batch_stats)   # mask from raw (_mask_mode)
        dw1 = ops.conv2d_k3_wgrad(cost, dc) if ctx.needs_input_grad[1] else None
        dcost = ops.conv2d_dgrad(dc, w1) if ctx.needs_input_grad[0] else None
        return (dcost, dw1) + _affine_grads(ctx, ctx.has[0], ctx.has[1], 2, dgamma, dbeta) + (dw2, None)


def _as3d_weight(w):
    """[Co, Ci, 3, 3] -> [Co, Ci, 3, 3, 3] with the 2-D taps on the middle plane: a 2-D layer seen by the 3-D stride-2 kernels."""
    w3 = torch.zeros(w.shape[:2] + (3, 3, 3), dtype=w.dtype, device=w.device)
    w3[:, :, 1] = w
    return w3


# Weight packs of the 2-D units across the two views of a training step.  The backbone runs the left and the right view through the
# same modules one after the other (backbones/PSMNet.py:119-131), so every unit packed its forward weights twice per step and
# built its data-gradient weights (a transpose, a flip, a copy, a pack) twice.  A pack now lives for a PHASE: the forward pack from
# the first forward call until the unit's next backward call, the data-gradient packs from the first backward call until the next
# forward call -- and, within its phase, while the weight matches its stamp (param_state: load_state_dict, an optimizer step).
def _phase_pack(unit, w, forward):
    mine, other = ("_dmb_pack_fwd", "_dmb_pack_bwd") if forward else ("_dmb_pack_bwd", "_dmb_pack_fwd")
    unit.__dict__[other] = None

    def make():
        return ops.pack_conv2d_weights(w) if forward else ops.conv2d_dgrad_packs(w, unit.dilation)
    if not _pack_group_enabled or torch.cuda.is_current_stream_capturing():
        unit.__dict__[mine] = None
        return make()
    return param_state.cached(unit, mine, (unit[0].weight,), make)


class Conv2dUnitFn(torch.autograd.Function):
    """y = act(BN(conv2d(x)) (+ skip)) of one FusedConv2d unit of the 2-D networks (layers/basic_layers.py:31-46,105-123):
    kernel 1 | 3, stride 1 | 2, dilation 1 | 2.  Stride-1 gradients run on the 2-D kernels; the few stride-2 layers borrow the
    3-D stride-2 kernels with a depth of one."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, skip, unit, relu, carry_x=False, carry_skip=False):
        x_in = x
        x = x.contiguous()
        w = weight.detach().contiguous()
        C, k, s, d = unit.out_planes, unit.kernel_size, unit.stride, unit.dilation
        if k == 5:
            if s != 2 or d != 1:
                raise NotImplementedError("training path of FusedConv2d: 5x5 layers are stride 2")
        elif k not in (1, 3) or d not in (1, 2, 4, 8) or (s == 2 and d != 1):
            raise NotImplementedError("training path of FusedConv2d: kernel 1|3, dilation 1|2|4|8, stride 2 only without dilation")
        sc, sh = _bias_as_shift(bias)
        raw = ops.conv2d(x, _phase_pack(unit, w, True), C, k, s, d, sc, sh, None, False)
        return _unit_forward_tail(ctx, unit, raw, x, w, x_in, gamma, beta, bias, skip, relu, carry_x, carry_skip)

    @staticmethod
    def backward(ctx, *grads):
        unit = ctx.unit
        unit.__dict__["_dmb_pack_fwd"] = None     # any backward call ends the forward phase of the unit's packs (_phase_pack)
        dc, dx_acc, x, w, bn_grads = _unit_backward_head(ctx, grads)
        k, s, d = unit.kernel_size, unit.stride, unit.dilation
        dw = dx = None
        if ctx.needs_input_grad[1]:
            if k == 5:     # 5x5 stride 2 = 3x3 stride 1 on the space-to-depth input (GC-Net's first layer)
                dw = _k5s2_wgrad(x, dc)
            elif s == 1:
                dw = ops.conv2d_wgrad(x, dc, k, d)
            elif k == 3:   # stride 2: the 3-D stride-2 weight gradient at depth 1, middle plane of its taps
                dw = ops.conv3d_k3s2_wgrad(x.unsqueeze(2), dc.unsqueeze(2))[:, :, 1].contiguous()
            else:          # 1x1, stride 2: a 1x1 layer on the even positions
                dw = ops.conv2d_wgrad(x[:, :, ::2, ::2].contiguous(), dc, 1, 1)
        if ctx.needs_input_grad[0]:
            if k == 5:
                dx = _k5s2_dgrad(dc, _k5s2_as_k3(w), x)
            elif s == 1:
                dx = ops.conv2d_dgrad(dc, w, d, residual=dx_acc, packs=_phase_pack(unit, w, False))
                dx_acc = None
            elif k == 3:
                dx = ops.conv3d_k3_dgrad(dc.unsqueeze(2), _as3d_weight(w), 2, (1,) + tuple(x.shape[2:])).squeeze(2)
            else:
                dx = torch.zeros_like(x)
                dx[:, :, ::2, ::2] = ops.conv2d_dgrad(dc, w, 1)
            if dx_acc is not None:   # the forms without a skip operand in their data-gradient launch
                dx = dx + dx_acc
        return _unit_backward_tail(ctx, dx, dw, bn_grads)


def conv2d_unit(unit, x, residual=None, relu=False):
    return _apply_carried(Conv2dUnitFn, unit, x, residual, relu)


class BareConv1x1Fn(torch.autograd.Function):
    """nn.Conv2d(C, Co, 1, bias=False) (the last layer of the PSMNet backbone, backbones/PSMNet.py:61-62)."""

    @staticmethod
    def forward(ctx, x, weight):
        x = x.contiguous()
        w = weight.detach().contiguous()
        ctx.save_for_backward(x, w)
        return ops.conv2d(x, ops.pack_conv2d_weights(w), w.shape[0], 1)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        return (ops.conv2d_dgrad(dy, w) if ctx.needs_input_grad[0] else None,
                ops.conv2d_wgrad(x, dy, 1, 1) if ctx.needs_input_grad[1] else None)


def _even(x):
    """x with a zero row / column appended to an odd height / width.  A 5x5 stride-2 layer (padding 2) reads that row or column as
    padding anyway, so it has the same outputs on the even-sized input; its data gradient there is sliced off again."""
    H, W = x.shape[2], x.shape[3]
    return torch.nn.functional.pad(x, (0, W % 2, 0, H % 2)) if H % 2 or W % 2 else x


def _space_to_depth(x):
    """[B, C, H, W] (even H, W) -> [B, 4C, H/2, W/2], channel order (c, row parity, column parity)."""
    B, C, H, W = x.shape
    return x.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(B, 4 * C, H // 2, W // 2)


def _depth_to_space(x):
    B, C4, H2, W2 = x.shape
    C = C4 // 4
    return x.view(B, C, 2, 2, H2, W2).permute(0, 1, 4, 2, 5, 3).reshape(B, C, 2 * H2, 2 * W2)


def _k5s2_as_k3(w):
    """A 5x5 stride-2 convolution (padding 2) IS a 3x3 stride-1 convolution (padding 1) on the space-to-depth input:
    x[2(o + A - 1) + r] meets w[2A + r] (A in 0..2, r in 0..1; the sixth tap is zero).  [Co, Ci, 5, 5] -> [Co, 4Ci, 3, 3]."""
    Co, Ci = w.shape[:2]
    w6 = torch.nn.functional.pad(w, (0, 1, 0, 1))
    return w6.view(Co, Ci, 3, 2, 3, 2).permute(0, 1, 3, 5, 2, 4).reshape(Co, 4 * Ci, 3, 3).contiguous()


def _k3_as_k5s2_grad(dw3, Ci):
    Co = dw3.shape[0]
    return dw3.view(Co, Ci, 2, 2, 3, 3).permute(0, 1, 4, 2, 5, 3).reshape(Co, Ci, 6, 6)[:, :, :5, :5].contiguous()


def _k5s2_wgrad(x, dc):
    """Weight gradient [Co, Ci, 5, 5] of a 5x5 stride-2 layer: that of the 3x3 layer on the space-to-depth input, folded back."""
    return _k3_as_k5s2_grad(ops.conv2d_wgrad(_space_to_depth(_even(x)).contiguous(), dc, 3, 1), x.shape[1])


def _k5s2_dgrad(dc, w3, x):
    """Data gradient of a 5x5 stride-2 layer with the 3x3 weight ``w3 = _k5s2_as_k3(w)``, cut back to an odd-sized ``x``."""
    return _depth_to_space(ops.conv2d_dgrad(dc, w3))[:, :, :x.shape[2], :x.shape[3]].contiguous()


class BareConv2dFn(torch.autograd.Function):
    """A bare nn.Conv2d with bias (backbones/StereoNet.py:26-27,76: 5x5 stride 2 or 3x3 stride 1; edge_aware.py:42 with its skip
    add and ReLU): y = act(conv(x) + bias (+ skip)).  The 5x5 stride-2 layers take their gradients through the equivalent 3x3
    stride-1 layer on the space-to-depth input."""

    @staticmethod
    def forward(ctx, x, weight, bias, skip, relu):
        x = x.contiguous()
        w = weight.detach().contiguous()
        Co, k = w.shape[0], w.shape[2]
        stride = 2 if k == 5 else 1
        b = bias.detach().contiguous() if bias is not None else None
        raw = ops.conv2d(x, ops.pack_conv2d_weights(w), Co, k, stride, 1, None, b, None, False)
        one, zero = _const(1.0, Co, x.device), _const(0.0, Co, x.device)
        if relu:
            y = ops.bn_act(raw, one, zero, skip, True)
        elif skip is not None:
            y = ops.bn_act(raw, one, zero, skip, False)
        else:
            y = raw
        ctx.relu, ctx.has = bool(relu), (bias is not None, skip is not None)
        ctx.save_for_backward(x, w, raw, y if relu and skip is not None else None, one, zero)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, raw, y, one, zero = ctx.saved_tensors
        has_bias, has_skip = ctx.has
        dy = dy.contiguous()
        need_dres = has_skip and ctx.needs_input_grad[3]
        dc, _, dsum, dres = ops.bn_act_bwd(dy, raw, y, one, zero, zero, one, _mask_mode(1 if ctx.relu else 0, has_skip), False,
                                           want_dres=need_dres and ctx.relu)
        if need_dres and not ctx.relu:
            dres = dy
        k = w.shape[2]
        dx = dw = None
        if k == 5:
            w3 = _k5s2_as_k3(w)
            if ctx.needs_input_grad[1]:
                dw = _k5s2_wgrad(x, dc)
            if ctx.needs_input_grad[0]:
                dx = _k5s2_dgrad(dc, w3, x)
        else:
            if ctx.needs_input_grad[1]:
                dw = ops.conv2d_wgrad(x, dc, k, 1)
            if ctx.needs_input_grad[0]:
                dx = ops.conv2d_dgrad(dc, w)
        return dx, dw, (dsum if has_bias and ctx.needs_input_grad[2] else None), (dres if need_dres else None), None


class BilinearScaleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, out_hw, mult):
        x = x.contiguous()
        ctx.hw, ctx.mult = tuple(x.shape[2:]), float(mult)
        return ops.bilinear_scale(x, tuple(out_hw), mult)

    @staticmethod
    def backward(ctx, dy):
        return ops.bilinear_scale_bwd(dy.contiguous(), ctx.hw, ctx.mult), None, None


class AvgPool2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        x = x.contiguous()
        ctx.k, ctx.hw = int(k), tuple(x.shape[2:])
        return ops.avgpool2d(x, k)

    @staticmethod
    def backward(ctx, dy):
        return ops.avgpool2d_bwd(dy.contiguous(), ctx.hw, ctx.k), None


class BilinearAcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, out_hw):
        x = x.contiguous()
        ctx.hw = tuple(x.shape[2:])
        return ops.bilinear_ac(x, tuple(out_hw))

    @staticmethod
    def backward(ctx, dy):
        return ops.bilinear_ac_bwd(dy.contiguous(), ctx.hw), None


class SoftArgminFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, values, alpha):
        cost = cost.contiguous()
        disp = ops.soft_argmin(cost, list(values), alpha, True)
        ctx.save_for_backward(cost, disp)
        ctx.values, ctx.alpha = tuple(values), float(alpha)
        return disp

    @staticmethod
    def backward(ctx, ddisp):
        cost, disp = ctx.saved_tensors
        return ops.soft_argmin_bwd(cost, disp, ddisp.contiguous(), list(ctx.values), ctx.alpha), None, None


# ---------------------------------------------------------------------------------------------- DeepPruner's sampler
PATCH_MATCH_BWD_MAX_W = 1024   # dmb_patch_match_step_bwd_f32 (DMB_PATCH_MATCH_BWD_MAX_W): 8 channel rows of W floats in LDS


def _refuse_double_backward(what):
    """Called first thing in a ``backward``.  Grad mode is on there only when the caller asked for a graph of the backward itself
    (``create_graph=True``): the launches below record none, so a second-order term would be dropped silently -- whether or not
    the upstream gradient itself requires one (a gradient penalty's does not).  Refuse instead."""
    if torch.is_grad_enabled():
        raise NotImplementedError("%s: double backward (a gradient of the gradient, create_graph=True) is not implemented on the "
                                  "HIP path" % what)


def _refuse_cpu(what, *tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise ops._lib.DmbLibraryError("%s: an operand lives on %s: the dmb HIP path only runs on a GPU (cuda/hip) tensor and "
                                           "has no CPU fallback" % (what, t.device))


class PatchMatchFn(torch.autograd.Function):
    """PatchMatch (disp_samplers/utils/patch_match.py:305-361) under autograd on csrc/patch_match.hip.  The forward is
    PatchMatch.forward's ``2 * iterations`` launches (the same bits) and keeps the [B, P, H, W] noise ENTERING each half-iteration
    -- nothing else; the backward runs dmb_patch_match_step_bwd_f32 over the steps in reverse, each recomputing its candidates
    and costs from that noise, and returns the gradients of ``left``, ``right`` and the initial ``noise`` (the last d_noise_in).
    The range is the constant ``bounds``, or two [B, 1, H, W] maps taken as constants (no gradient for them)."""

    @staticmethod
    def forward(ctx, left, right, noise, min_disparity, max_disparity, bounds, iterations, temperature):
        B, _, H, W = left.shape
        P = noise.shape[1]
        out = torch.empty((B, P + 2, H, W), dtype=torch.float32, device=left.device)
        steps, noises = 2 * int(iterations), []
        for step in range(steps):
            last = step == steps - 1
            noises.append(noise)
            _, noise = ops.patch_match_step(left, right, noise, min_disparity, max_disparity, vertical=step % 2 == 1,
                                            temperature=temperature, bounds=bounds, want_noise=not last, out=out if last else None)
        ctx.has_maps = min_disparity is not None
        ctx.save_for_backward(left, right, *(((min_disparity, max_disparity) if ctx.has_maps else ()) + tuple(noises)))
        ctx.bounds, ctx.temperature = tuple(bounds), temperature
        return out

    @staticmethod
    def backward(ctx, dout):
        _refuse_double_backward("PatchMatch")
        left, right = ctx.saved_tensors[:2]
        lo, hi = ctx.saved_tensors[2:4] if ctx.has_maps else (None, None)
        noises = ctx.saved_tensors[4 if ctx.has_maps else 2:]
        dL = dR = None
        gS, gN = dout.contiguous(), None     # [B, P + 2, H, W]: the two ends are the range, constants here
        for step in range(len(noises) - 1, -1, -1):
            dL, dR, gN = ops_deeppruner.patch_match_step_bwd(left, right, noises[step], lo, hi, grad_samples=gS, grad_noise=gN,
                                                  vertical=step % 2 == 1, temperature=ctx.temperature, bounds=ctx.bounds,
                                                  grad_left_acc=dL, grad_right_acc=dR)
            gS = None                        # only the last half-iteration's samples are an output
        need = ctx.needs_input_grad
        return (dL if need[0] else None, dR if need[1] else None, gN if need[2] else None, None, None, None, None, None)


class UniformSamplesFn(torch.autograd.Function):
    """Stage "post" (DeepPruner.py:48-66, 99-115) under autograd: dmb_deeppruner_uniform_samples_f32 and its backward, one
    elementwise launch each."""

    @staticmethod
    def forward(ctx, min_disparity, max_disparity, sample_number, max_disp):
        ctx.save_for_backward(min_disparity, max_disparity)
        ctx.max_disp = max_disp
        return ops.deeppruner_uniform_samples(min_disparity, max_disparity, sample_number, max_disp)

    @staticmethod
    def backward(ctx, dout):
        _refuse_double_backward("UniformSampler")
        lo, hi = ctx.saved_tensors
        glo, ghi = ops_deeppruner.deeppruner_uniform_samples_bwd(lo, hi, dout.contiguous(), ctx.max_disp)
        return (glo if ctx.needs_input_grad[0] else None, ghi if ctx.needs_input_grad[1] else None, None, None)


def deeppruner_sampler(sampler, stage, left, right, min_disparity=None, max_disparity=None, noise=None):
    """Differentiable forward of a DeepPrunerSampler (whose own ``forward`` stays inference only): stage "pre" is PatchMatch over
    [0, max_disp] with gradients for ``left``, ``right`` and ``noise``; any other stage is the range head and the uniform sampler
    with gradients for the two maps.  Counts, temperature, iterations and ``max_disp`` are the sampler's."""
    if stage == 'pre':
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (min_disparity, max_disparity)):
            raise NotImplementedError("deeppruner_sampler: stage 'pre' ignores the range maps (DeepPruner.py:176-184); a gradient "
                                      "for PatchMatch's range is not implemented on the HIP path")
        pm = sampler.patch_match
        if left.dim() != 4:
            raise ValueError("PatchMatch: features must be [B, C, H, W], got %s" % (tuple(left.shape),))
        B, _, H, W = left.shape
        if H < 2 or W < 2:
            raise NotImplementedError("PatchMatch: H, W >= 2 (the reference divides by size - 1), got %dx%d" % (H, W))
        if W > PATCH_MATCH_BWD_MAX_W:   # refuse here, not inside backward()
            raise NotImplementedError("PatchMatch under autograd: feature maps wider than %d columns have no backward on the HIP "
                                      "path (the forward alone has no such limit: run it under torch.no_grad())"
                                      % PATCH_MATCH_BWD_MAX_W)
        P = pm.disparity_sample_number - 2
        if noise is not None:
            noise = pm.check_noise(noise, left)
        _refuse_cpu("deeppruner_sampler", left, right)
        if noise is None:
            noise = torch.rand((B, P, H, W), dtype=torch.float32, device=left.device)
        return PatchMatchFn.apply(left.contiguous(), right.contiguous(), noise.contiguous(), None, None,
                                  (0.0, float(sampler.max_disp)), pm.iterations, pm.temperature)
    if min_disparity is None or max_disparity is None:
        raise ValueError("DeepPrunerSampler: stage %r needs min_disparity and max_disparity" % (stage,))
    _refuse_cpu("deeppruner_sampler", min_disparity, max_disparity)
    return UniformSamplesFn.apply(min_disparity.contiguous(), max_disparity.contiguous(),
                                  sampler.uniform_sampler.disparity_sample_number, sampler.max_disp)


# ---------------------------------------------------------------------------------------------- DeepPruner's aggregator
class _SingleBackwardFn(torch.autograd.Function):
    """Identity on the output of a function built from the units above.  Its backward runs before any of theirs, so a double
    backward is refused before the first launch."""

    @staticmethod
    def forward(ctx, y, what):
        ctx.what = what
        return y.view_as(y)

    @staticmethod
    def backward(ctx, dy):
        _refuse_double_backward(ctx.what)
        return dy, None


def _hw_hourglass_units(hourglass, x, skip):
    levels = []
    for k in (1, 2, 3):                                   # down (hw_hourglass.py:79-94): relu(bn(conv)) + its own input
        down = conv_unit(getattr(hourglass, "conv%d_a" % k), x, None, True)
        x = conv_unit(getattr(hourglass, "conv%d_b" % k), down, down, "pre")
        levels.append(x)
    for k in (3, 2):                                      # up (:97-100): bn(deconv) + the level above, no ReLU
        x = conv_unit(getattr(hourglass, "conv%d_d" % k), x, levels[k - 2], False)
    return conv_unit(hourglass.conv1_d, x, skip, False)   # :103 (+ the caller's skip)


def _check_hw_volume(what, x, planes):
    if x.dim() != 5 or x.shape[1] != planes or x.shape[3] % 8 or x.shape[4] % 8:
        raise ValueError("%s: input must be [B, %d, D, H, W] with H and W multiples of 8, got %s" % (what, planes, tuple(x.shape)))


def hw_hourglass(hourglass, x, skip=None):
    """Differentiable forward of an HWHourglass (whose own ``forward`` stays inference only): the nine units in the order and with
    the adds of HWHourglass.forward, each on ConvUnitFn -- the stride-(1, 2, 2) ones with the (1, 2, 2) kernels of the other
    direction as their data gradients and the (1, 2, 2) weight gradient (csrc/wgrad.hip).  ``skip``: the caller's
    ``hourglass(x) + x``, added by conv1_d.  Every BatchNorm follows its own ``training`` flag."""
    _check_hw_volume("HWHourglass", x, hourglass.in_planes)
    if skip is not None and tuple(skip.shape) != tuple(x.shape):
        raise ValueError("HWHourglass: skip shape %s != input shape %s" % (tuple(skip.shape), tuple(x.shape)))
    _refuse_cpu("hw_hourglass", x, skip)
    with carry_scope():
        return _SingleBackwardFn.apply(_hw_hourglass_units(hourglass, x, skip), "hw_hourglass")


def deeppruner_aggregator(aggregator, raw_cost):
    """Differentiable forward of a DeepPrunerAggregator (whose own ``forward`` stays inference only): dres0, dres1, the hourglass
    plus its input, the classifier (DeepPruner.py:47-59).  Returns ``[cost]``, [B, D, H, W]."""
    if hasattr(raw_cost, "materialize"):
        raw_cost = raw_cost.materialize()
    _check_hw_volume("DeepPrunerAggregator", raw_cost, aggregator.in_planes)
    _refuse_cpu("deeppruner_aggregator", raw_cost)
    with carry_scope():
        x = raw_cost
        for unit in tuple(aggregator.dres0) + tuple(aggregator.dres1):            # DeepPruner.py:49-51
            x = conv_unit(unit, x, None, True)
        x = _hw_hourglass_units(aggregator.dres2, x, x)                           # :54, the add in conv1_d
        x = conv_unit(aggregator.classify[0], x, None, True)
        head = aggregator.classify[1]
        cost = HeadConvFn.apply(x, head.weight, head.bias, None)                  # :57
        return [_SingleBackwardFn.apply(cost, "deeppruner_aggregator").squeeze(1)]


# ---------------------------------------------------------------------------------------------- DeepPruner's cost processor
class SmallConv5x5Fn(torch.autograd.Function):
    """y = act(BN(conv5x5(x) + bias)) of one SmallConv5x5 unit (stride 1, padding 2, 1 .. 16 channels) on the unit skeleton.  Raw
    convolution: dmb_conv2d_k5_small_f32 with the bias as its shift and no ReLU; BatchNorm2d by batch statistics, running statistics
    or none, following its own ``training`` flag.  Backward: the weight gradient is plan form 6 of csrc/wgrad.hip; the data gradient
    is the forward kernel on mirrored, channel-exchanged weights (stride 1 with padding 2 is its own adjoint geometry)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, skip, unit, relu, carry_x=False, carry_skip=False):
        x_in = x
        x = x.contiguous()
        w = weight.detach().contiguous()
        raw = ops_deeppruner.conv2d_k5_small(x, w, None, bias.detach().contiguous() if bias is not None else None, False)
        return _unit_forward_tail(ctx, unit, raw, x, w, x_in, gamma, beta, bias, skip, relu, carry_x, carry_skip)

    @staticmethod
    def backward(ctx, *grads):
        _refuse_double_backward("SmallConv5x5")
        dc, dx_acc, x, w, bn_grads = _unit_backward_head(ctx, grads)
        dw = dx = None
        if ctx.needs_input_grad[1]:
            dw = ops.conv2d_wgrad(x, dc, 5, 1)
        if ctx.needs_input_grad[0]:
            dx = ops_deeppruner.conv2d_k5_small(dc, w.flip(2, 3).transpose(0, 1).contiguous())
            if dx_acc is not None:
                dx = dx + dx_acc
        return _unit_backward_tail(ctx, dx, dw, bn_grads)


def small_conv5x5(unit, x):
    """Differentiable forward of a SmallConv5x5 (whose own ``forward`` stays inference only)."""
    _refuse_cpu("small_conv5x5", x)
    return _apply_carried(SmallConv5x5Fn, unit, x, None, unit.has_relu)


class SoftArgminSampledFn(torch.autograd.Function):
    """disp = sum_d softmax(cost)_d * sample_d over per-pixel samples (alpha = 1, normalised): cost, sample [B, D, H, W] ->
    [B, 1, H, W].  Forward: dmb_soft_argmin_sampled_f32.  Backward, composed of torch ops on the device (D <= 14 planes; its share
    of the step is in docs/design/21): with p = softmax(cost, 1), d_cost = d_disp * p * (sample - disp), d_sample = d_disp * p."""

    @staticmethod
    def forward(ctx, cost, sample, normalize=True):
        if not normalize:
            raise NotImplementedError("SoftArgminSampledFn: only the normalised form (softmax over the samples) has a backward")
        cost, sample = cost.contiguous(), sample.contiguous()
        disp = ops.soft_argmin_sampled(cost, sample, 1.0, True)
        ctx.save_for_backward(cost, sample, disp)
        return disp

    @staticmethod
    def backward(ctx, ddisp):
        _refuse_double_backward("soft_argmin_sampled")
        cost, sample, disp = ctx.saved_tensors
        gp = torch.softmax(cost, 1) * ddisp
        d_cost = gp * (sample - disp) if ctx.needs_input_grad[0] else None
        return d_cost, (gp if ctx.needs_input_grad[1] else None), None


class DeepPrunerVolumeFn(torch.autograd.Function):
    """ops_deeppruner.deeppruner_volume under autograd: [B, 2C + 1 + 2P, D, H, W] = cat(fast_cat_fms(left, right, sample), sample,
    min_feature on every plane, max_feature on every plane).  Backward, a composition: the first 2C channels through the sampled
    volume's adjoint (dmb_fast_fms_bwd_f32, which wants them dense: one copy), the sample channel added to the sampler's column
    derivative, the range features' gradients summed over the planes in ascending plane order."""

    @staticmethod
    def forward(ctx, left, right, sample, min_feature, max_feature):
        left, right, sample = left.contiguous(), right.contiguous(), sample.contiguous()
        vol = ops_deeppruner.deeppruner_volume(left, right, sample, min_feature, max_feature)
        ctx.save_for_backward(left, right, sample)
        ctx.P = 0 if min_feature is None else min_feature.shape[1]
        return vol

    @staticmethod
    def backward(ctx, dvol):
        _refuse_double_backward("deeppruner_volume")
        left, right, sample = ctx.saved_tensors
        need, C, P, D = ctx.needs_input_grad, left.shape[1], ctx.P, sample.shape[1]
        dL = dR = dS = dmin = dmax = None
        if need[0] or need[1] or need[2]:
            dL, dR, dS = ops.fast_fms_bwd(left, right, sample, dvol[:, :2 * C].contiguous(), wrt_samples=need[2])
        if need[2]:
            dS = dS + dvol[:, 2 * C]

        def over_planes(c0):
            acc = dvol[:, c0:c0 + P, 0].clone()
            for d in range(1, D):                       # ascending plane order
                acc += dvol[:, c0:c0 + P, d]
            return acc
        if P and need[3]:
            dmin = over_planes(2 * C + 1)
        if P and need[4]:
            dmax = over_planes(2 * C + 1 + P)
        return dL if need[0] else None, dR if need[1] else None, dS, dmin, dmax


def _check_volume_inputs(what, left, right, sample):
    if left.dim() != 4 or sample.dim() != 4:
        raise ValueError("%s: features [B, C, H, W] and per-pixel samples [B, D, H, W] expected, got %s and %s"
                         % (what, tuple(left.shape), tuple(sample.shape)))
    if left.shape[-1] > FAST_FMS_BWD_MAX_W:   # refuse here, not inside backward(): the adjoint keeps 2 x 8 rows of W floats in LDS
        raise NotImplementedError("%s under autograd: feature maps wider than %d columns have no backward on the HIP path (the "
                                  "forward alone has no such limit: run it under torch.no_grad())" % (what, FAST_FMS_BWD_MAX_W))


def deeppruner_volume(left, right, sample, min_feature=None, max_feature=None):
    """Differentiable ``ops_deeppruner.deeppruner_volume``: gradients for the two feature maps, the per-pixel samples and the two
    range feature maps."""
    _check_volume_inputs("deeppruner_volume", left, right, sample)
    _refuse_cpu("deeppruner_volume", left, right, sample, min_feature, max_feature)
    return DeepPrunerVolumeFn.apply(left, right, sample.float(), min_feature, max_feature)


def confidence_range_predictor(predictor, raw_cost, disparity_sample):
    """Differentiable forward of a ConfidenceRangePredictor (whose own ``forward`` stays inference only) -> (min_disparity,
    max_disparity, min_disparity_feature, max_disparity_feature): the trunk, the two (hourglass, 16 -> 32, 32 -> 1) branches, two
    soft arg-mins over the samples and the four 5x5 convolutions (DeepPruner.py:88-119).  The trunk's output and each range cost
    have two consumers: everything runs inside one carry scope."""
    _check_hw_volume("ConfidenceRangePredictor", raw_cost, predictor.in_planes)
    _refuse_cpu("confidence_range_predictor", raw_cost, disparity_sample)
    what = "confidence_range_predictor"
    with carry_scope():
        x = raw_cost
        for unit in tuple(predictor.dres0) + tuple(predictor.dres1):                          # DeepPruner.py:88-89
            x = conv_unit(unit, x, None, True)
        costs = []
        for branch in (predictor.min_disparity_predictor, predictor.max_disparity_predictor):  # :91-96
            y = conv_unit(branch[1], _hw_hourglass_units(branch[0], x, None), None, True)
            costs.append(HeadConvFn.apply(y, branch[2].weight, branch[2].bias, None).squeeze(1))
        outs = (small_conv5x5(predictor.min_disparity_conv, SoftArgminSampledFn.apply(costs[0], disparity_sample)),   # :98-110
                small_conv5x5(predictor.max_disparity_conv, SoftArgminSampledFn.apply(costs[1], disparity_sample)),
                small_conv5x5(predictor.min_disparity_feature_conv, costs[0]),                                       # :112-113
                small_conv5x5(predictor.max_disparity_feature_conv, costs[1]))
        return tuple(_SingleBackwardFn.apply(o, what) for o in outs)


def deeppruner_processor(processor, stage, left, right, disparity_sample, min_disparity_feature=None, max_disparity_feature=None):
    """Differentiable forward of a DeepPrunerProcessor (whose own ``forward`` stays inference only).  Stage "pre": the volume, then
    the range predictor's four maps; any other stage: the volume with the two range feature maps, the aggregator, the soft arg-min,
    both up-samplings and the two 5x5 convolutions -> [disparity, disparity_feature] (DeepPruner.py:190-234).  Gradients reach
    ``left``, ``right``, ``disparity_sample``, the two feature maps and every parameter."""
    what = "deeppruner_processor"
    _check_volume_inputs(what, left, right, disparity_sample)
    if left.shape[2] % 8 or left.shape[3] % 8:
        raise ValueError("%s: H and W must be multiples of 8 (the hourglass halves them three times), got %s" % (what, tuple(left.shape)))
    _refuse_cpu(what, left, right, disparity_sample, min_disparity_feature, max_disparity_feature)
    if stage == 'pre':
        raw_cost = deeppruner_volume(left, right, disparity_sample)                                           # DeepPruner.py:192-195
        return confidence_range_predictor(processor.confidence_range_predictor, raw_cost, disparity_sample)
    raw_cost = deeppruner_volume(left, right, disparity_sample, min_disparity_feature, max_disparity_feature)  # :192-195, 204-208
    cost = deeppruner_aggregator(processor.cost_aggregator, raw_cost)[0]
    disparity = SoftArgminSampledFn.apply(cost, disparity_sample)                                             # :216-218
    H, W = cost.shape[2:]
    disparity = BilinearScaleFn.apply(disparity, (2 * H, 2 * W), 2.0)                                         # :221 (see the module)
    disparity_feature = BilinearScaleFn.apply(cost, (2 * H, 2 * W), 1.0)                                      # :224
    return [_SingleBackwardFn.apply(small_conv5x5(processor.disparity_conv, disparity), what),
            _SingleBackwardFn.apply(small_conv5x5(processor.disparity_feature_conv, disparity_feature), what)]


# ---------------------------------------------------------------------------------------------- DeepPruner's refinement
class RefineHeadFn(torch.autograd.Function):
    """The tail of a refinement stage, y = up2(2 * relu(conv3x3_{Ci -> 1}(x) + init)) (disp_refinement/DeepPruner.py:40-42, 87),
    Ci <= 16, from launches the library already has.  Forward: r = relu(conv(x) + init) on dmb_preact_conv_f32 (no prologue, the
    residual epilogue: one ascending (ci, ky, kx) fmaf chain from 0, the chain of csrc/refine_head.hip), then
    dmb_bilinear_scale_f32 by two -- the bits of ops_deeppruner.refine_head_up2.  Backward: the up-sampling's adjoint, the ReLU
    mask from r (r > 0 IS conv + init > 0), d_init = dc, dx = the 1 -> Ci convolution of dc with the mirrored weight on the same
    direct kernel, dw = plan form 7 of csrc/wgrad.hip."""

    @staticmethod
    def forward(ctx, x, weight, init):
        x, init = x.contiguous(), init.contiguous()
        w = weight.detach().contiguous()
        r = ops.preact_conv(x, w, residual=init)          # (with a residual the epilogue is relu(sum + residual))
        ctx.save_for_backward(x, w, r)
        H, W = r.shape[2:]
        return ops.bilinear_scale(r, (2 * H, 2 * W), 2.0)

    @staticmethod
    def backward(ctx, dy):
        _refuse_double_backward("refinement_head")
        x, w, r = ctx.saved_tensors
        need = ctx.needs_input_grad
        dr = ops.bilinear_scale_bwd(dy.contiguous(), tuple(r.shape[2:]), 2.0)
        one, zero = _const(1.0, 1, r.device), _const(0.0, 1, r.device)
        dc = ops.bn_act_bwd(dr, r, r, one, zero, zero, one, True, False)[0]     # dr where r > 0: the mask from the output
        # the mirrored, channel-exchanged weight [Ci, 1, 3, 3]: with one output channel the exchange is a view of the flipped copy
        dx = ops.preact_conv(dc, w.flip(2, 3).view(w.shape[1], 1, 3, 3)) if need[0] else None
        dw = ops.conv2d_wgrad(x, dc, 3, 1) if need[1] else None
        return dx, dw, (dc if need[2] else None)


def refinement_head(block, init_disp, guide):
    """Differentiable tail of a RefinementHeand (whose own ``forward`` stays inference only): ``guide`` is the output of the six
    conv + BatchNorm + ReLU layers [B, Ci <= 16, H, W], ``init_disp`` [B, 1, H, W] -> [B, 1, 2H, 2W].  Gradients reach both and
    ``block.classify.weight``."""
    w = block.classify.weight
    if guide.dim() != 4 or guide.shape[1] != w.shape[1] or guide.shape[1] > ops_deeppruner.REFINE_HEAD_MAX_C \
            or tuple(init_disp.shape) != (guide.shape[0], 1) + tuple(guide.shape[2:]):
        raise ValueError("refinement_head: guide [B, %d, H, W] and init_disp [B, 1, H, W] expected, got %s and %s"
                         % (w.shape[1], tuple(guide.shape), tuple(init_disp.shape)))
    _refuse_cpu("refinement_head", guide, init_disp, w)
    return RefineHeadFn.apply(guide, w, init_disp)


class _PlainCtx:
    """What the static ``forward`` / ``backward`` of ``Conv2dUnitFn`` and ``RefineHeadFn`` read and write of an autograd context
    (``needs_input_grad``, ``save_for_backward`` / ``saved_tensors``, ``set_materialize_grads``, plain attributes), for a caller
    that runs several of them inside ONE Function.  What it keeps of autograd's saved-tensor rules: a tensor modified in place
    between forward and backward is refused (its ``_version`` is compared, as autograd does).  What it does not: the tensors are
    released when the owning node dies, not right after backward -- so a second backward over the same graph runs, with or
    without ``retain_graph`` -- and ``torch.autograd.graph.saved_tensors_hooks`` (checkpointing, offload) do not see them."""

    def __init__(self, needs_input_grad):
        self.needs_input_grad, self._saved, self._versions = tuple(needs_input_grad), (), ()

    def save_for_backward(self, *tensors):
        self._saved, self._versions = tensors, tuple(None if t is None else t._version for t in tensors)

    @property
    def saved_tensors(self):
        for t, v in zip(self._saved, self._versions):
            if t is not None and t._version != v:
                raise RuntimeError("one of the variables needed for gradient computation has been modified by an inplace operation: "
                                   "a %s tensor saved by a refinement stage is at version %d, expected %d" % (tuple(t.shape), t._version, v))
        return self._saved

    def set_materialize_grads(self, flag):
        pass


class RefineStageFn(torch.autograd.Function):
    """One refinement stage after its guide is built: the six conv + BatchNorm + ReLU layers and the head, as ONE node of the
    autograd graph.  The forward is ``Conv2dUnitFn.forward`` six times and ``RefineHeadFn.forward``, the backward their
    ``backward``s in reverse -- the same launches in the same order with the same bits as eight nodes chained through
    ``conv2d_unit`` and ``refinement_head`` (a plain chain: no tensor inside has a second consumer, so there is nothing to carry).
    At a 256 x 512 crop the interpreter, not the GPU, sets the stage's pace (docs/design/22), and a Python autograd node costs it
    more than any kernel of the stage takes.  The units run on ``_PlainCtx`` objects: its docstring states what that keeps and what
    it gives up of autograd's saved-tensor rules (tests/test_deeppruner_refinement_bwd_gpu.py pins both).  Inputs: the block (its units supply geometry and BatchNorm buffers), guide, init, per unit (weight, bias,
    gamma, beta), the classifier's weight.  Double backward is refused before the first launch."""

    @staticmethod
    def forward(ctx, block, guide, init, *params):
        need = ctx.needs_input_grad
        x, ctx.units = guide, []
        for i, unit in enumerate(block.conv):
            c = _PlainCtx((need[1] if i == 0 else True,) + tuple(need[3 + 4 * i:7 + 4 * i]) + (False,) * 5)
            x = Conv2dUnitFn.forward(c, x, *params[4 * i:4 * i + 4], None, unit, True)
            ctx.units.append(c)
        ctx.head = _PlainCtx((True, need[-1], need[2]))
        return RefineHeadFn.forward(ctx.head, x, params[-1], init)

    @staticmethod
    def backward(ctx, dy):
        _refuse_double_backward("deeppruner_refinement")
        dx, d_classify, d_init = RefineHeadFn.backward(ctx.head, dy)
        grads = ()
        for c in reversed(ctx.units):
            out = Conv2dUnitFn.backward(c, dx)
            dx, grads = out[0], tuple(out[1:5]) + grads          # (dw, dbias, dgamma, dbeta) of the unit
        return (None, dx, d_init) + grads + (d_classify,)


def deeppruner_refinement(refinement, disps, low_ref_group_fms):
    """Differentiable forward of a DeepPrunerRefinement (whose own ``forward`` stays inference only): per stage the guide
    cat(low_ref_group_fms[i], init_disp) (DeepPruner.py:83), then the six conv + BatchNorm + ReLU layers and the head as one
    ``RefineStageFn``.  Returns a new list, the incoming maps and one map per stage, reversed: the better map first.  Gradients
    reach every ``low_ref_group_fms[i]``, the incoming disparity (the guide's last channel, the head's ``init`` and its own place in
    the list) and every parameter.  Every BatchNorm follows its own ``training`` flag."""
    what = "deeppruner_refinement"
    disps = list(disps)
    _refuse_cpu(what, *disps, *low_ref_group_fms[:refinement.num])
    for i in range(refinement.num):
        init_disp, fms, block = disps[-1], low_ref_group_fms[i], refinement.refine_blocks[i]
        if fms.dim() != 4 or tuple(init_disp.shape) != (fms.shape[0], 1) + tuple(fms.shape[2:]):
            raise ValueError("%s: stage %d takes features [B, C, H, W] and a disparity [B, 1, H, W], got %s and %s"
                             % (what, i, tuple(fms.shape), tuple(init_disp.shape)))
        head_in = block.classify.weight.shape[1]
        if fms.shape[1] + 1 != block.in_planes or head_in != block.conv[-1].out_planes or head_in > ops_deeppruner.REFINE_HEAD_MAX_C:
            raise ValueError("%s: stage %d is built for %d guide channels and a head of at most %d, got features %s"
                             % (what, i, block.in_planes, ops_deeppruner.REFINE_HEAD_MAX_C, tuple(fms.shape)))
        params = []
        for unit in block.conv:                                                   # :38-39
            conv, _, gamma, beta = _unit_params(unit)
            params += [conv.weight, conv.bias, gamma, beta]
        guide = torch.cat((fms, init_disp), 1)                                    # :83
        disps.append(RefineStageFn.apply(block, guide, init_disp, *params, block.classify.weight))   # :40-42, 85-87
    disps.reverse()
    return disps


def wants_grad(module, *tensors):
    """True when a forward call must take the unit-by-unit path of this file instead of the fused inference kernels:
    (a) the module is in training mode (batch statistics and running-buffer updates are training-mode semantics with or
    without autograd, e.g. a validation pass under torch.no_grad() inside train()); or (b) gradients are enabled and
    something on this call can receive one -- an input that already carries a gradient, or one of the module's OWN
    parameters (``model.train(); model.backbone.eval()`` freezes the backbone's BatchNorm statistics, not its weights: with
    the reference's plain nn modules those weights still get gradients, and so they do here; each BatchNorm follows its own
    ``training`` flag).  Under torch.no_grad() -- how the reference's tools run evaluation, and what
    GeneralizedStereoModel's eval branch enters itself -- an eval-mode module stays on the fused kernels, unless (c) its
    BatchNorm keeps no running buffers: that normalises with batch statistics in every mode, which no folded scale / shift
    can express."""
    if module.training:
        return True
    if getattr(module, "has_bn", False) and _batch_stats(module[1]):
        return True
    if not torch.is_grad_enabled():
        return False
    if any(t is not None and getattr(t, "requires_grad", False) for t in tensors):
        return True
    if any(p.requires_grad for p in module.parameters()):
        _warn_eval_on_training_path(module)
        return True
    return False


_warned_eval_path = [False]


def _warn_eval_on_training_path(module):
    """An eval-mode module called with gradients enabled and trainable parameters takes the unit-by-unit autograd path (full-size
    activations saved, no fused volume / regression kernels): several times the memory and latency of the inference path.
    That is what the reference's nn modules would do too, but it is easy to hit by accident -- say so once."""
    if not _warned_eval_path[0]:
        _warned_eval_path[0] = True
        import warnings
        warnings.warn("%s is in eval mode but gradients are enabled and its parameters require grad: taking the autograd "
                      "(training) path.  Wrap inference in torch.no_grad() -- as GeneralizedStereoModel's eval branch does -- to "
                      "stay on the fused inference kernels." % type(module).__name__, stacklevel=3)
