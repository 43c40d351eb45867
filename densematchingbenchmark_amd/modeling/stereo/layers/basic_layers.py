"""3-D conv + BatchNorm (+ReLU) units of the aggregators, backed by the fused HIP kernels.

Mirrors the factories of dmb/modeling/stereo/layers/basic_layers.py:68-100,160-177 -- same names, same argument
order, same ``state_dict`` keys (``<unit>.0.weight``, ``<unit>.1.running_mean`` ...) -- but every unit is a
``FusedConv3d`` whose forward is ONE kernel launch: convolution with BatchNorm folded into a per-channel
scale/shift, optional residual add and ReLU in the epilogue.  torch.nn modules are kept only as parameter
containers so that reference checkpoints load with ``load_state_dict``.  In training mode (or when an input carries a
gradient) the same units run as autograd Functions on the HIP kernels (train_fn.py).  No CPU fallback.
"""
import torch
import torch.nn as nn

from .... import ops, ops_head, param_state
from . import train_fn

__all__ = ["FusedConv3d", "HeadConv3d", "HeadDeconv3d", "conv3d_bn", "conv3d_bn_relu", "deconv3d_bn", "deconv3d_bn_relu",
           "bn_parts", "classifier_branch", "fold_batch_norm"]


def fold_batch_norm(bn, conv_bias, out_planes, device):
    """Eval-mode BN as y = x * scale + shift, folded in FP64 and rounded once:
    scale = gamma / sqrt(var + eps), shift = beta - mean * scale (+ conv_bias * scale)."""
    if bn is None:
        if conv_bias is None:
            return None, None
        return torch.ones(out_planes, dtype=torch.float32, device=device), conv_bias.detach().float().contiguous()
    if bn.running_mean is None or bn.running_var is None:
        raise NotImplementedError("fold_batch_norm: a BatchNorm without running statistics (track_running_stats=False) "
                                  "normalises with batch statistics in eval() too; it has no folded form")
    var = bn.running_var.detach().double()
    mean = bn.running_mean.detach().double()
    gamma = bn.weight.detach().double() if bn.affine else torch.ones_like(var)
    beta = bn.bias.detach().double() if bn.affine else torch.zeros_like(var)
    scale = gamma / torch.sqrt(var + bn.eps)
    shift = beta - mean * scale
    if conv_bias is not None:
        shift = shift + conv_bias.detach().double() * scale
    return scale.float().contiguous(), shift.float().contiguous()


def bn_parts(bn):
    """The tensors a folded BatchNorm is derived from (none without one).  ``num_batches_tracked`` is among them: the
    training-mode kernel rewrites ``running_mean`` / ``running_var`` through raw device pointers (their ``_version`` does not
    move), but every such forward bumps ``num_batches_tracked`` in place."""
    return () if bn is None else (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked)


def epoch_on_mode_switch(module, mode):
    """Called from train(mode) of the fused modules: a switch between training and evaluation advances the parameter epoch
    (param_state), so the first forward after it re-folds whatever the versions say."""
    if bool(mode) != module.training:
        param_state.bump_param_epoch()


class FusedConv3d(nn.Sequential):
    """Sequential(Conv3d | ConvTranspose3d, [BatchNorm3d], [ReLU]) executed as one fused HIP kernel.

    kernel 3 / padding 1 convolutions with stride 1, 2 or (1, 2, 2), and kernel 3 / padding 1 transposed convolutions with
    stride 2 / output_padding 1 or stride (1, 2, 2) / output_padding (0, 1, 1) (the only forms the aggregators use; ``stride``
    and ``output_padding`` may be ints or 3-tuples, (1, 1, 1) meaning 1 as hw_hourglass.py:36-39 writes it).
    ``forward(x, residual=None)`` computes ``act(BN(conv(x)) + residual)`` where ``act`` is ReLU iff the unit has one or
    ``relu=True`` is passed (hourglass.py:67-70,78-81 apply the ReLU after the skip add).

    The (1, 2, 2) forms and the 16-output-channel forms (DeepPruner's HWHourglass, csrc/conv3d_hw.hip) are inference-only."""

    HW = (1, 2, 2)

    def __init__(self, batch_norm, in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=True,
                 relu=False, transposed=False, output_padding=0):
        layers = []
        stride = self._triple(stride)
        output_padding = self._triple(output_padding)
        if transposed:
            form = (kernel_size, stride, padding, output_padding)
            if form == (3, self.HW, 1, (0, 1, 1)):
                if out_planes not in (16, 32, 64):
                    raise NotImplementedError("HIP transposed conv with stride (1, 2, 2): 16, 32 or 64 output channels, got %d"
                                              % out_planes)
            elif form != (3, 2, 1, 1):
                raise NotImplementedError("HIP transposed conv: only kernel 3, padding 1 with stride 2, output_padding 1 or "
                                          "stride (1, 2, 2), output_padding (0, 1, 1)")
            layers.append(nn.ConvTranspose3d(in_planes, out_planes, kernel_size, stride=stride, padding=padding,
                                             output_padding=output_padding, bias=bias))
        else:
            if kernel_size != 3 or padding != 1 or dilation != 1 or stride not in (1, 2, self.HW):
                raise NotImplementedError("HIP conv3d: only kernel 3, padding 1, dilation 1, stride 1, 2 or (1, 2, 2)")
            if stride == self.HW and out_planes not in (16, 32, 64, 128):
                raise NotImplementedError("HIP conv3d with stride (1, 2, 2): 16, 32, 64 or 128 output channels, got %d" % out_planes)
            if stride == 2 and out_planes == 16:
                raise NotImplementedError("HIP conv3d: 16 output channels with stride 1 or (1, 2, 2) only")
            layers.append(nn.Conv3d(in_planes, out_planes, kernel_size, stride=stride, padding=padding,
                                    dilation=dilation, bias=bias))
        if batch_norm:
            layers.append(nn.BatchNorm3d(out_planes))
        if relu:
            layers.append(nn.ReLU(inplace=True))
        super().__init__(*layers)
        self.in_planes, self.out_planes, self.stride = in_planes, out_planes, stride
        self.transposed, self.has_bn, self.has_relu = transposed, bool(batch_norm), bool(relu)
        # the forms of csrc/conv3d_hw.hip: no backward, never the bf16x6 path
        self.hw_form = stride == self.HW or (out_planes == 16 and not (transposed and stride == 2))

    @staticmethod
    def _triple(v):
        """An int, or a 3-tuple collapsed to an int when its entries agree ((1, 1, 1) -> 1)."""
        if isinstance(v, (tuple, list)):
            v = tuple(int(e) for e in v)
            if len(v) != 3:
                raise NotImplementedError("HIP conv3d: stride / output_padding must be an int or a 3-tuple, got %s" % (v,))
            return v[0] if v[0] == v[1] == v[2] else v
        return v

    def train(self, mode=True):
        epoch_on_mode_switch(self, mode)
        return super().train(mode)

    def _batch_stats(self):
        """Training mode, or a BatchNorm that normalises with batch statistics in every mode (no running buffers)."""
        return self.training or (self.has_bn and train_fn._batch_stats(self[1]))

    def _prepacked(self):
        conv = self[0]
        bn = self[1] if self.has_bn else None

        def make():
            w = conv.weight.detach()
            wp = ops.pack_deconv3d_weights(w) if self.transposed else ops.pack_conv3d_weights(w)
            return (wp,) + fold_batch_norm(bn, conv.bias, self.out_planes, w.device)
        return param_state.cached(self, "_dmb_packed", (conv.weight, conv.bias) + bn_parts(bn), make)

    def forward(self, x, residual=None, relu=None, skip=None):
        """``residual`` is added BEFORE the activation (hourglass.py:67-81), ``skip`` AFTER it (GC-Net,
        aggregators/GCNet.py:108-116: ``layer34(cost33 + cost29)`` -- the add runs in layer33's epilogue)."""
        act = self.has_relu if relu is None else relu
        if getattr(x, "kind", None) == "gwc_cat":   # LazyGwcCatVolume: correlation channels 3-D, concat channels as 2-D maps
            G = x.num_groups
            if (residual is None and skip is None and not self.transposed and self.stride == 1 and not self._batch_stats()
                    and x.shape[1] == self.in_planes and G % 2 == 0 and self.out_planes == 32
                    and ops.catconv_applicable(x.reference_fm, x.target_fm, x.disp_idx, self.out_planes)):
                def make():
                    w = self[0].weight.detach()
                    return ops.pack_conv3d_weights(w[:, :G].contiguous()), ops.catconv_pack(w[:, G:].contiguous(), "cat")
                wp_g, packs = param_state.cached(self, "_dmb_packed_gwc", (self[0].weight,), make)
                _, scale, shift = self._prepacked()
                # convolution is linear in its input channels: relu(scale * (conv(gwc) + maps(cat)) + shift), the maps' part
                # entering the 3-D kernel's epilogue as its residual operand, already scaled
                part = ops.catconv_first(x.reference_fm, x.target_fm, len(x.disp_idx), packs, scale, None, False)
                return ops.conv3d_k3(x.correlation_part(), wp_g, self.out_planes, scale, shift, part, 1, act)
            x = x.materialize()
        elif hasattr(x, "materialize"):   # LazyCatVolume: the concatenation volume as a description
            if (residual is None and skip is None and not self.transposed and self.stride == 1
                    and x.shape[1] == self.in_planes
                    and ops.catconv_applicable(x.reference_fm, x.target_fm, x.disp_idx, self.out_planes)):
                if getattr(x, "differentiable", False) or self._batch_stats():
                    # training path: the 2-D form in the forward pass, the volume only inside the backward pass
                    return train_fn.cat_conv_unit(self, x, act)
                _, scale, shift = self._prepacked()
                return ops.catconv_first(x.reference_fm, x.target_fm, len(x.disp_idx), self._prepacked_cat(x.kind), scale, shift, act)
            x = x.materialize()
        if skip is not None:
            if residual is not None:
                raise ValueError("FusedConv3d: residual and skip are mutually exclusive")
            residual, act = skip, ("pre" if act else False)
        if train_fn.wants_grad(self, x, residual):
            if self.hw_form:
                raise NotImplementedError("FusedConv3d: the stride-(1, 2, 2) and 16-output-channel units are inference-only "
                                          "(no backward); call eval() and run under torch.no_grad()")
            # training / differentiable path: conv, BatchNorm statistics, epilogue and their backward
            # passes as separate HIP launches under torch.autograd
            return train_fn.conv_unit(self, x, residual, act)
        wp, scale, shift = self._prepacked()
        if self.transposed:
            if self.stride == self.HW:
                return ops.deconv3d_k3s2(x, wp, self.out_planes, scale, shift, residual, act, stride=self.HW)
            return ops.deconv3d_k3s2(x, wp, self.out_planes, scale, shift, residual, act)
        if self.hw_form:
            return ops.conv3d_k3(x, wp, self.out_planes, scale, shift, residual, self.stride, act)
        if ops.conv3d_mode() == "bf16x6" and ops.conv3d_x6_applicable(x, self.out_planes, self.stride):
            return ops.conv3d_k3_x6(x, self._prepacked_x6(), self.out_planes, scale, shift, residual, act)   # opt-in only
        return ops.conv3d_k3(x, wp, self.out_planes, scale, shift, residual, self.stride, act)

    def _prepacked_cat(self, kind):
        w = self[0].weight
        return param_state.cached(self, "_dmb_packed_" + kind, (w,), lambda: ops.catconv_pack(w.detach(), kind))

    def _prepacked_x6(self):
        w = self[0].weight
        return param_state.cached(self, "_dmb_packed_x6", (w,), lambda: ops.pack_conv3d_x6_weights(w.detach()))


class HeadConv3d(nn.Conv3d):
    """nn.Conv3d(C, 1, 3, 1, 1) classifier head (PSMNet.py:46, StereoNet.py:39) on the single-channel HIP kernel;
    ``forward(x, residual=None)`` fuses the cumulative cost add of PSMNet.py:71-72."""

    def __init__(self, in_planes, bias=False):
        super().__init__(in_planes, 1, kernel_size=3, stride=1, padding=1, bias=bias)

    def train(self, mode=True):
        epoch_on_mode_switch(self, mode)
        return super().train(mode)

    def forward(self, x, residual=None):
        if hasattr(x, "materialize"):   # a lazy volume reaching a head directly (an aggregator without trunk layers)
            x = x.materialize()
        if train_fn.wants_grad(self, x, residual):
            return train_fn.HeadConvFn.apply(x, self.weight, self.bias, residual)
        return ops.conv3d_k3_c1(x, self.weight.detach(), self.bias_value(), residual)

    def bias_value(self):
        if self.bias is None:
            return 0.0
        # one device->host read per weight load, not per call
        return param_state.cached(self, "_dmb_bias", (self.bias,), lambda: float(self.bias.detach().cpu()[0]))


def classifier_branch(unit, head, x, residual=None):
    """``head(unit(x), residual)`` for a classifier branch (PSMNet.py:44-54,70-72): FusedConv3d 32 -> 32 + BN + ReLU, then
    HeadConv3d 32 -> 1.  In eval mode with no gradient wanted, exact conv3d arithmetic, split-K semantics on and a launch that
    takes the 48 x 4 row-pair tile, both layers run as ONE convolution launch whose 32-channel output never reaches memory
    (ops_head.conv3d_k3_head); otherwise the two launches."""
    if _head_fuses(unit, head, x, residual):
        wp, scale, shift = unit._prepacked()
        return ops_head.conv3d_k3_head(x, wp, _packed_head(head), scale, shift, head.bias_value(), residual, True)
    return head(unit(x), residual=residual)


def _head_fuses(unit, head, x, residual=None):
    return (isinstance(unit, FusedConv3d) and isinstance(head, HeadConv3d) and torch.is_tensor(x) and x.dim() == 5
            and unit.out_planes == 32 and head.in_channels == 32 and unit.stride == 1 and not unit.transposed and unit.has_relu
            and not train_fn.wants_grad(unit, x) and not train_fn.wants_grad(head, x, residual)
            and ops_head.conv3d_k3_head_applicable(x))


def _packed_head(head):
    return param_state.cached(head, "_dmb_packed_head", (head.weight,), lambda: ops_head.pack_conv3d_head_weights(head.weight.detach()))


def classifier_chain(branches, xs):
    """The costs of a chain of classifier branches, ``cost_k = head_k(unit_k(x_k)) + cost_{k-1}`` (PSMNet.py:70-72), where EVERY
    branch takes the fused form of ``classifier_branch``: the convolutions leave their partial sums in one workspace each and one
    finishing pass writes all levels (ops_head.conv3d_head_chain_finish) -- the same bits as the branches one after the other.
    ``branches``: (unit, head) pairs, ``xs``: their inputs of one shape.  Returns [N, B, 1, D, H, W], or None where a branch does
    not take the fused form (the caller then runs ``classifier_branch`` per level)."""
    if not 1 <= len(branches) <= 4 or any(not torch.is_tensor(x) or x.shape != xs[0].shape for x in xs):
        return None
    if not all(_head_fuses(unit, head, x) for (unit, head), x in zip(branches, xs)):
        return None
    wss = []
    for (unit, head), x in zip(branches, xs):
        wp, scale, shift = unit._prepacked()
        wss.append(ops_head.conv3d_k3_head_partial(x, wp, _packed_head(head), scale, shift, True))
    B, _, D, H, W = xs[0].shape
    return ops_head.conv3d_head_chain_finish(wss, [head.bias_value() for _, head in branches], (B, D, H, W))


class HeadDeconv3d(nn.ConvTranspose3d):
    """nn.ConvTranspose3d(C, Co<=32, 3, stride 2, padding 1, output_padding 1, bias) without BN / activation (GC-Net's
    1-channel output layer, aggregators/GCNet.py:63-67) on the MFMA transposed kernel with zero-padded weight rows."""

    def __init__(self, in_planes, out_planes):
        super().__init__(in_planes, out_planes, kernel_size=3, stride=2, padding=1, output_padding=1)

    def forward(self, x):
        if train_fn.wants_grad(self, x):
            return train_fn.HeadDeconvFn.apply(x, self.weight, self.bias)
        wp, bias = param_state.cached(self, "_dmb_packed", (self.weight, self.bias), lambda: (
            ops.pack_deconv3d_weights(self.weight.detach()), self.bias.detach().float().contiguous()))
        return ops.deconv3d_k3s2(x, wp, self.out_channels, None, bias, None, False)


def conv3d_bn(batchNorm, in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=True):
    """basic_layers.py:68-83."""
    return FusedConv3d(batchNorm, in_planes, out_planes, kernel_size, stride, padding, dilation, bias, relu=False)


def conv3d_bn_relu(batchNorm, in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=True):
    """basic_layers.py:160-177."""
    return FusedConv3d(batchNorm, in_planes, out_planes, kernel_size, stride, padding, dilation, bias, relu=True)


def deconv3d_bn(batchNorm, in_planes, out_planes, kernel_size=4, stride=2, padding=1, output_padding=0, bias=True):
    """basic_layers.py:86-100."""
    return FusedConv3d(batchNorm, in_planes, out_planes, kernel_size, stride, padding, 1, bias, relu=False,
                       transposed=True, output_padding=output_padding)


def deconv3d_bn_relu(batchNorm, in_planes, out_planes, kernel_size=4, stride=2, padding=1, output_padding=0, bias=True):
    """basic_layers.py:180-197."""
    return FusedConv3d(batchNorm, in_planes, out_planes, kernel_size, stride, padding, 1, bias, relu=True,
                       transposed=True, output_padding=output_padding)
