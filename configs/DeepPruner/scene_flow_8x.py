# DeepPruner "fast" on SceneFlow: features at 1/8 (layer3 strides too; the backbone also returns its 64-channel 1/4 and 32-channel
# 1/2 maps), PatchMatch over 0 .. 24 at that scale, two refinement stages: at 1/4 guided by 64 + 9 + 1 channels, at 1/2 by 32 + 1.
# Eval at 576x960 (a multiple of 64 at 1/8 for the hourglass).  The model class is reached by import (models/DeepPruner.py,
# apis.init_model); build_model refuses the meta-architecture.
import os, runpy
_c = runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "_common.py"))
task = 'stereo'
max_disp = 192
_P, _N, _C = 14, 9, 32     # PatchMatch samples (both ends included), uniform samples, feature channels


def _l1(weights):
    return dict(l1_loss=dict(max_disp=max_disp, weights=weights, weight=1.0),
                quantile_loss=dict(max_disp=max_disp, theta=0.05, weight=1.0))


_SCALE = 8
model = dict(
    meta_architecture="DeepPruner",
    max_disp=max_disp,
    batch_norm=True,
    backbone=dict(type="FastDeepPruner", in_planes=3),
    disp_sampler=dict(type="DeepPruner", max_disp=max_disp // _SCALE, propagation_filter_size=3, iterations=3, temperature=7,
                      patch_match_disparity_sample_number=_P, uniform_disparity_sample_number=_N),
    cost_processor=dict(
        type="DeepPruner", patch_match_disparity_sample_number=_P, uniform_disparity_sample_number=_N,
        confidence_range_predictor=dict(in_planes=2 * _C + 1, hourglass_in_planes=16),
        cost_aggregator=dict(type="DeepPruner", in_planes=2 * _C + 2 * _P + 1, hourglass_in_planes=16),
    ),
    disp_refinement=dict(type='DeepPruner', in_planes_list=[64 + _N + 1, _C + 1], num=2),
    losses=_l1((1.6, 1.3, 1.0, 0.7, 0.7)),
    eval=dict(lower_bound=0, upper_bound=max_disp, eval_occlusion=True, is_cost_return=False, is_cost_to_cpu=True),
)
data = dict(sparse=False, eval=dict(input_shape=[576, 960], mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375]))
dist_params = dict(backend='nccl')
