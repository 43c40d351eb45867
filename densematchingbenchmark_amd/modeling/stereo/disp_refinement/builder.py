"""Registry of the disparity refinements on the HIP path (the reference's disp_refinement/builder.py:5-9 also lists
AnyNet, whose refinement is reached through its own model here)."""
from ...registry import instantiate
from .DeepPruner import DeepPrunerRefinement
from .StereoNet import StereoNetRefinement

REFINEMENTS = dict(StereoNet=StereoNetRefinement, DeepPruner=DeepPrunerRefinement)


def build_disp_refinement(cfg):
    return instantiate(REFINEMENTS, cfg.model.disp_refinement, "disparity refinement", off_path=("AnyNet",),
                       batch_norm=cfg.model.batch_norm)
