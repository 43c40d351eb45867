# DeepPruner "best" on SceneFlow: features at 1/4 (the PSMNet-like backbone, which also returns its 1/2 map), PatchMatch over
# 0 .. 48 at that scale with 14 samples, 9 uniform samples inside the predicted range, one refinement stage guided by the 32-channel
# 1/2 map, the 9-channel disparity feature and the disparity itself.  Eval at 544x960.  The model class is reached by import
# (models/DeepPruner.py, apis.init_model); build_model refuses the meta-architecture.
import os, runpy
_c = runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "_common.py"))
task = 'stereo'
max_disp = 192
_P, _N, _C = 14, 9, 32     # PatchMatch samples (both ends included), uniform samples, feature channels


def _l1(weights):
    return dict(l1_loss=dict(max_disp=max_disp, weights=weights, weight=1.0),
                quantile_loss=dict(max_disp=max_disp, theta=0.05, weight=1.0))


_SCALE = 4
model = dict(
    meta_architecture="DeepPruner",
    max_disp=max_disp,
    batch_norm=True,
    backbone=dict(type="BestDeepPruner", in_planes=3),
    disp_sampler=dict(type="DeepPruner", max_disp=max_disp // _SCALE, propagation_filter_size=3, iterations=3, temperature=7,
                      patch_match_disparity_sample_number=_P, uniform_disparity_sample_number=_N),
    cost_processor=dict(
        type="DeepPruner", patch_match_disparity_sample_number=_P, uniform_disparity_sample_number=_N,
        confidence_range_predictor=dict(in_planes=2 * _C + 1, hourglass_in_planes=16),
        cost_aggregator=dict(type="DeepPruner", in_planes=2 * _C + 2 * _P + 1, hourglass_in_planes=16),
    ),
    disp_refinement=dict(type='DeepPruner', in_planes_list=[_C + _N + 1], num=1),
    losses=_l1((1.3, 1.0, 0.7, 0.7)),
    eval=dict(lower_bound=0, upper_bound=max_disp, eval_occlusion=True, is_cost_return=False, is_cost_to_cpu=True),
)
data = dict(sparse=False, eval=dict(input_shape=[544, 960], mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375]))
dist_params = dict(backend='nccl')
