"""Registry of the disparity samplers (the reference's disp_samplers/builder.py:3-19)."""
from ...registry import instantiate
from .DeepPruner import DeepPrunerSampler

SAMPLER = dict(DeepPruner=DeepPrunerSampler)


def build_disp_sampler(cfg):
    return instantiate(SAMPLER, cfg.model.disp_sampler, "disparity sampler", batch_norm=cfg.model.batch_norm)
