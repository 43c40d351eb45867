from .builder import REFINEMENTS, build_disp_refinement
from .DeepPruner import DeepPrunerRefinement, RefinementHeand
from .StereoNet import StereoNetRefinement

__all__ = ["REFINEMENTS", "build_disp_refinement", "StereoNetRefinement", "DeepPrunerRefinement", "RefinementHeand"]
