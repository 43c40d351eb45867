"""DeepPruner's disparity sampler on the HIP path (the reference's disp_samplers/DeepPruner.py and utils/patch_match.py).

Stage "pre": differentiable PatchMatch over the full range [0, max_disp] -- ``2 * iterations`` launches of one fused
propagate + evaluate kernel (dmb_patch_match_step_f32), the last of which writes the [B, P + 2, H, W] result with both ends of
the range in place.  Stage "post": the range head and the uniform sampler in one elementwise launch
(dmb_deeppruner_uniform_samples_f32).  No parameters.  These modules are inference only; the differentiable path is
``layers.train_fn.deeppruner_sampler(sampler, stage, ...)`` on the same kernels and their backward (docs/design/14).

The reference draws PatchMatch's initial noise inside the module; here ``noise=None`` draws it from torch's device generator
(``torch.manual_seed`` reproduces a call) and a given ``noise`` tensor [B, P, H, W] is used as it is and left untouched.
"""
import torch
import torch.nn as nn

from .... import ops


def _refuse_gradients(what, *tensors):
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        raise NotImplementedError("%s: an input requires a gradient, but this module is inference only (call it under "
                                  "torch.no_grad()); the backward of PatchMatch / the disparity sampler is reached through "
                                  "layers.train_fn.deeppruner_sampler(sampler, stage, ...)" % what)


class DisparitySampleRangeHead(nn.Module):
    """DeepPruner.py:8-68.  Stage "pre" is the constant range [0, max_disp] and stage "post" the ordered, stretched, halved and
    clamped range; both are computed inside the sampler's launches, so this module only carries ``max_disp``."""

    def __init__(self, max_disp):
        super().__init__()
        self.max_disp = max_disp

    def forward(self, *args, **kwargs):
        raise NotImplementedError("the range head runs fused inside DeepPrunerSampler's launches; it has no launch of its own")


class UniformSampler(nn.Module):
    """DeepPruner.py:71-115: ``disparity_sample_number`` samples per pixel, both ends of [min, max] included."""

    def __init__(self, disparity_sample_number=9):
        super().__init__()
        if not 2 <= disparity_sample_number <= ops.MAX_DISP_SAMPLES:
            raise NotImplementedError("UniformSampler: 2 .. %d samples, got %r" % (ops.MAX_DISP_SAMPLES, disparity_sample_number))
        self.disparity_sample_number = disparity_sample_number

    def forward(self, min_disparity, max_disparity, max_disp=None):
        _refuse_gradients("UniformSampler", min_disparity, max_disparity)
        return ops.deeppruner_uniform_samples(min_disparity, max_disparity, self.disparity_sample_number, max_disp)


class PatchMatch(nn.Module):
    """patch_match.py:256-361.  ``disparity_sample_number`` counts both ends of the range: P = disparity_sample_number - 2
    intervals carry one particle each."""

    def __init__(self, propagation_filter_size=3, disparity_sample_number=14, iterations=3, temperature=7):
        super().__init__()
        if propagation_filter_size != 3:
            raise NotImplementedError("PatchMatch: the fused step is built for propagation_filter_size 3, got %r"
                                      % (propagation_filter_size,))
        if int(iterations) != iterations or iterations < 1:
            raise NotImplementedError("PatchMatch: iterations must be an integer >= 1, got %r" % (iterations,))
        if not 1 <= disparity_sample_number - 2 <= ops.PATCH_MATCH_MAX_SAMPLES:
            raise NotImplementedError("PatchMatch: 3 .. %d samples (ends included), got %r"
                                      % (ops.PATCH_MATCH_MAX_SAMPLES + 2, disparity_sample_number))
        self.propagation_filter_size = propagation_filter_size
        self.disparity_sample_number = disparity_sample_number
        self.iterations = int(iterations)
        self.temperature = temperature

    def check_noise(self, noise, left):
        B, _, H, W = left.shape
        shape = (B, self.disparity_sample_number - 2, H, W)
        if not isinstance(noise, torch.Tensor) or tuple(noise.shape) != shape or noise.dtype != torch.float32 \
                or noise.device != left.device:
            raise ValueError("PatchMatch: noise must be a float32 tensor %s on %s, got %s" % (
                shape, left.device, "%s %s on %s" % (noise.dtype, tuple(noise.shape), noise.device)
                if isinstance(noise, torch.Tensor) else type(noise).__name__))
        return noise

    def forward(self, left, right, min_disparity=None, max_disparity=None, noise=None, bounds=(0.0, 0.0)):
        """The range is the two [B, 1, H, W] maps or, both None, the constants ``bounds`` on every pixel."""
        _refuse_gradients("PatchMatch", left, right, min_disparity, max_disparity, noise)
        if left.dim() != 4:
            raise ValueError("PatchMatch: features must be [B, C, H, W], got %s" % (tuple(left.shape),))
        B, _, H, W = left.shape
        if H < 2 or W < 2:
            raise NotImplementedError("PatchMatch: H, W >= 2 (the reference divides by size - 1), got %dx%d" % (H, W))
        P = self.disparity_sample_number - 2
        if noise is None:
            noise = torch.rand((B, P, H, W), dtype=torch.float32, device=left.device)
        else:
            noise = self.check_noise(noise, left)
        out = torch.empty((B, P + 2, H, W), dtype=torch.float32, device=left.device)
        steps = 2 * self.iterations
        for step in range(steps):
            last = step == steps - 1
            _, noise = ops.patch_match_step(left, right, noise, min_disparity, max_disparity, vertical=step % 2 == 1,
                                            temperature=self.temperature, bounds=bounds, want_noise=not last,
                                            out=out if last else None)
        return out


class DeepPrunerSampler(nn.Module):
    """DeepPruner.py:118-191.  ``forward(stage, left, right, min_disparity, max_disparity)``: stage "pre" ignores the two maps
    (full range, PatchMatch, ``patch_match_disparity_sample_number`` samples), any other stage is "post" (range head, uniform
    sampler, ``uniform_disparity_sample_number`` samples)."""

    def __init__(self, max_disp, batch_norm=True, propagation_filter_size=3, iterations=3, temperature=7,
                 patch_match_disparity_sample_number=14, uniform_disparity_sample_number=9):
        super().__init__()
        self.max_disp = max_disp
        self.batch_norm = batch_norm
        self.propagation_filter_size = propagation_filter_size
        self.iterations = iterations
        self.temperature = temperature
        self.patch_match_disparity_sample_number = patch_match_disparity_sample_number
        self.uniform_disparity_sample_number = uniform_disparity_sample_number
        self.disparity_sample_range = DisparitySampleRangeHead(max_disp=max_disp)
        self.patch_match = PatchMatch(propagation_filter_size=propagation_filter_size,
                                      disparity_sample_number=patch_match_disparity_sample_number,
                                      iterations=iterations, temperature=temperature)
        self.uniform_sampler = UniformSampler(disparity_sample_number=uniform_disparity_sample_number)

    def forward(self, stage, left, right, min_disparity=None, max_disparity=None, noise=None):
        if stage == 'pre':
            return self.patch_match(left, right, noise=noise, bounds=(0.0, float(self.max_disp)))
        if min_disparity is None or max_disparity is None:
            raise ValueError("DeepPrunerSampler: stage %r needs min_disparity and max_disparity" % (stage,))
        _refuse_gradients("DeepPrunerSampler", left, right)
        return self.uniform_sampler(min_disparity, max_disparity, max_disp=self.max_disp)
