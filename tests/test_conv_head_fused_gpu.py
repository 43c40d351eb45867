"""The fused classifier tail (``ops_head.conv3d_k3_head``: csrc/conv3d_s1s2.hip, conv3d_s1_kernel on S1HeadCfg + conv3d_head_finish_kernel)
against the two launches it replaces (``ops.conv3d_k3`` 32 -> 32 + BN + ReLU, then ``ops.conv3d_k3_c1`` 32 -> 1 + residual).

Shapes, the smallest at which tiles (4 x 4 x 48 voxels) and their one-voxel halos can go wrong:
  [1, 32, 4, 4, 48]   one tile: every halo partial sum belongs to a voxel outside the volume and is dropped;
  [1, 32, 8, 8, 96]   two tiles on each axis: interior seams in z, y and x, corner voxels summed from eight tiles;
  [2, 32, 5, 6, 96]   partial tiles in z and y (voxels the convolution computes outside the volume must not reach the head),
                      batch 2, with the residual.
Truth is the FP64 evaluation of the same two layers on the same FP32 operands (folded BatchNorm included) by torch's double
kernels; the reference is the two-launch path, held to the form of bench.py::PARITY_CONTRACT:
  max |fused - fp64| <= max(1e-4, 1.25 max |two launches - fp64|)   and   mean |fused - fp64| <= mean |two launches - fp64|.
No margin on the mean: the fused head adds 27 chains of 32 terms (then at most eight tile sums) where the two launches add one
chain of 864, and a blocked sum's rounding error is the smaller one -- measured values are printed before the assertions.

The model-level policy (``basic_layers.classifier_branch``) is tested at [1, 32, 32, 64, 96], the smallest volume of these widths for
which the 32 -> 32 launch picks the 48 x 4 tile on 256 CUs (256 tiles: one per CU), and at W = 40, where it does not."""
import pytest
import torch
import torch.nn.functional as F

from densematchingbenchmark_amd import ops, ops_head
from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers import HeadConv3d, classifier_branch, conv3d_bn_relu

pytestmark = pytest.mark.gpu

SHAPES = {"one_tile": ((1, 32, 4, 4, 48), False), "seams": ((1, 32, 8, 8, 96), False), "partial_b2_res": ((2, 32, 5, 6, 96), True)}


def _modules(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    unit, head = conv3d_bn_relu(True, 32, 32, 3, 1, 1, bias=False), HeadConv3d(32, bias=False)
    with torch.no_grad():
        unit[0].weight.copy_(torch.randn(unit[0].weight.shape, generator=g) / (32 * 27) ** 0.5)
        unit[1].weight.copy_(torch.rand(32, generator=g) + 0.5)
        unit[1].bias.copy_(torch.randn(32, generator=g) * 0.2)
        unit[1].running_mean.copy_(torch.randn(32, generator=g) * 0.2)
        unit[1].running_var.copy_(torch.rand(32, generator=g) + 0.5)
        head.weight.copy_(torch.randn(head.weight.shape, generator=g) / (32 * 27) ** 0.5 * 4.0)
    return unit.to(dev).eval(), head.to(dev).eval()


def _inputs(shape, with_res, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    res = torch.randn((shape[0], 1) + tuple(shape[2:]), generator=g) if with_res else None
    return x.to(dev), (res.to(dev) if with_res else None)


def _fused(unit, head, x, res):
    wp, scale, shift = unit._prepacked()
    return ops_head.conv3d_k3_head(x, wp, ops_head.pack_conv3d_head_weights(head.weight.detach()), scale, shift, 0.0, res, True)


def _two_launches(unit, head, x, res, single_chain=False):
    """``single_chain``: on the single-chain kernels whatever the launch's size (conv3d_s1_kernel + conv3d_c1v_kernel, the pair a
    full-size step runs), not the split-K forms a launch this small would take."""
    before = ops.split_k()
    ops.set_split_k(before and not single_chain)
    try:
        with torch.no_grad():
            return head(unit(x), residual=res)
    finally:
        ops.set_split_k(before)


def _fp64(unit, head, x, res):
    _, scale, shift = unit._prepacked()
    y = F.conv3d(x.cpu().double(), unit[0].weight.detach().cpu().double(), padding=1)
    y = torch.relu(y * scale.cpu().double().view(1, 32, 1, 1, 1) + shift.cpu().double().view(1, 32, 1, 1, 1))
    c = F.conv3d(y, head.weight.detach().cpu().double(), padding=1)
    return c if res is None else c + res.cpu().double()


@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_head_meets_the_parity_contract_against_the_two_launches(dev, name):
    shape, with_res = SHAPES[name]
    unit, head = _modules(dev)
    x, res = _inputs(shape, with_res, dev)
    assert ops.split_k() and ops_head.pack_conv3d_head_weights(head.weight.detach()).numel() == 1024
    fused, two, truth = _fused(unit, head, x, res), _two_launches(unit, head, x, res, single_chain=True), _fp64(unit, head, x, res)
    assert fused.shape == two.shape == truth.shape and bool(torch.isfinite(fused).all())
    e_f, e_t = (fused.cpu().double() - truth).abs(), (two.cpu().double() - truth).abs()
    print("%s: max |fused - fp64| %.3e (two launches %.3e), mean %.4e (two launches %.4e), max |fused - two| %.3e" % (
        name, e_f.max().item(), e_t.max().item(), e_f.mean().item(), e_t.mean().item(), (fused - two).abs().max().item()))
    assert e_f.max().item() <= max(1e-4, 1.25 * e_t.max().item())
    assert e_f.mean().item() <= e_t.mean().item()
    assert torch.equal(fused, _fused(unit, head, x, res)), "two calls differ"


def test_fused_head_without_activation_or_affine(dev):
    """relu = 0 and NULL scale / shift: the head of the raw convolution."""
    unit, head = _modules(dev, seed=3)
    x, _ = _inputs((1, 32, 5, 8, 52), False, dev, seed=4)     # W % 48 != 0: a partial tile in x
    wp, _, _ = unit._prepacked()
    got = ops_head.conv3d_k3_head(x, wp, ops_head.pack_conv3d_head_weights(head.weight.detach()), None, None, 0.25, None, False)
    y = F.conv3d(x.cpu().double(), unit[0].weight.detach().cpu().double(), padding=1)
    truth = F.conv3d(y, head.weight.detach().cpu().double(), padding=1) + 0.25
    ops.set_split_k(False)      # the reference: the single-chain kernel pair, not the split-K forms of a launch this small
    try:
        two = ops.conv3d_k3_c1(ops.conv3d_k3(x, wp, 32), head.weight.detach(), 0.25)
    finally:
        ops.set_split_k(True)
    e_f, e_t = (got.cpu().double() - truth).abs(), (two.cpu().double() - truth).abs()
    print("raw: max %.3e (two launches %.3e), mean %.4e (two launches %.4e)" % (e_f.max().item(), e_t.max().item(), e_f.mean().item(), e_t.mean().item()))
    assert e_f.max().item() <= max(1e-4, 1.25 * e_t.max().item()) and e_f.mean().item() <= e_t.mean().item()


def test_hip_graph_replay_equals_eager(dev):
    shape, _ = SHAPES["partial_b2_res"]
    unit, head = _modules(dev)
    x, res = _inputs(shape, True, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm-up off the default stream: weight packing, per-device attributes
        _fused(unit, head, x, res)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _fused(unit, head, x, res)
    x2, res2 = _inputs(shape, True, dev, seed=7)
    x.copy_(x2)
    res.copy_(res2)
    graph.replay()
    torch.cuda.synchronize()
    got = captured.clone()
    assert torch.equal(got, _fused(unit, head, x2, res2))


def test_model_policy_takes_the_fused_form_where_the_tile_is_picked(dev):
    unit, head = _modules(dev)
    x, _ = _inputs((1, 32, 32, 64, 96), False, dev)
    assert ops_head.conv3d_k3_head_applicable(x)
    with torch.no_grad():
        got = classifier_branch(unit, head, x)
    assert torch.equal(got, _fused(unit, head, x, None))
    two = _two_launches(unit, head, x, None)
    assert not torch.equal(got, two) and (got - two).abs().max().item() < 1e-4     # another sum order, the same numbers


def test_reproducibility_switch_restores_the_two_launches(dev, single_chain):
    unit, head = _modules(dev)
    x, _ = _inputs((1, 32, 32, 64, 96), False, dev)
    assert not ops_head.conv3d_k3_head_applicable(x)
    with torch.no_grad():
        assert torch.equal(classifier_branch(unit, head, x), _two_launches(unit, head, x, None))


def test_a_width_that_does_not_take_the_tile_falls_back(dev):
    unit, head = _modules(dev)
    x, res = _inputs((1, 32, 8, 8, 40), True, dev)
    assert not ops_head.conv3d_k3_head_applicable(x)
    with torch.no_grad():
        assert torch.equal(classifier_branch(unit, head, x, res), _two_launches(unit, head, x, res))


def test_rows_that_are_not_16_bytes_are_refused(dev):
    from densematchingbenchmark_amd._lib import DmbLibraryError
    unit, head = _modules(dev)
    x, _ = _inputs((1, 32, 4, 4, 46), False, dev)
    with pytest.raises((DmbLibraryError, RuntimeError)):
        _fused(unit, head, x, None)
