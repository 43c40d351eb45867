# AnyNet (anytime stereo) on SceneFlow: backbone with C = 1 base channel, an initial guess at 1/16 over 12 disparities, two warp
# stages at 1/8 and 1/4 over residuals -2 .. 2, and the SPN refinement at 1/4.  Eval at 544x960.
import os, runpy
_c = runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "_common.py"))
task = 'stereo'
max_disp = 192
C = 1
_stages = ['init_guess', 'warp_level_8', 'warp_level_4']


def _per_stage(init, warp):
    return dict(init_guess=init, warp_level_8=warp, warp_level_4=warp)


model = dict(
    meta_architecture="AnyNet",
    max_disp=max_disp,
    batch_norm=True,
    stage=_stages,
    backbone=dict(type="AnyNet", in_planes=3, C=C, block_num=2),
    cost_processor=dict(
        type='AnyNet',
        cost_computation=dict(type="fast_mode", max_disp=_per_stage(max_disp // 16, 5), start_disp=_per_stage(0, -2),
                              dilation=_per_stage(1, 1)),
        cost_aggregator=dict(type="AnyNet", in_planes=dict(init_guess=8 * C, warp_level_8=4 * C, warp_level_4=2 * C),
                             agg_planes=_per_stage(16, 4), num=4),
    ),
    disp_predictor=dict(type="FASTER", max_disp=_per_stage(max_disp // 16, 5), start_disp=_per_stage(0, -2),
                        dilation=_per_stage(1, 1), alpha=1.0, normalize=True),
    disp_refinement=dict(type='AnyNet', in_planes=3, spn_planes=8),
    losses=dict(l1_loss=dict(max_disp=max_disp, weights=(1.0, 1.0, 0.5, 0.25), weight=1.0)),
    eval=dict(lower_bound=0, upper_bound=max_disp, eval_occlusion=True, is_cost_return=False, is_cost_to_cpu=True),
)
data = dict(sparse=False, eval=dict(input_shape=[544, 960], mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375]))
eval_disparity_id = [0, 1, 2, 3]
dist_params = dict(backend='nccl')
