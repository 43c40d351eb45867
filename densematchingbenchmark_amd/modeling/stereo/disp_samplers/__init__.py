from .builder import SAMPLER, build_disp_sampler
from .DeepPruner import DeepPrunerSampler, DisparitySampleRangeHead, PatchMatch, UniformSampler

__all__ = ["SAMPLER", "build_disp_sampler", "DeepPrunerSampler", "DisparitySampleRangeHead", "PatchMatch", "UniformSampler"]
