"""One finishing pass for PSMNet's three classifier levels (csrc/conv3d_s1s2.hip:
conv3d_head_chain_finish_kernel; ops_head.conv3d_k3_head_partial / conv3d_head_chain_finish; basic_layers.classifier_chain;
aggregators/PSMNet.py).  Nothing here has a tolerance: the chain only changes WHO adds a voxel's terms and when, so every
comparison is ``torch.equal``.

Chain finish: N = 1, 2, 3 convolution launches into N workspaces + one chain finish against N successive ``conv3d_k3_head`` calls
with the previous level's cost as the residual, through the C entry points (the wrappers of ops_head call them whatever tile the
estimate prefers).  Shapes, the smallest at which tiles (4 x 4 x 48 voxels) and their one-voxel halos can go wrong:
  [1, 32, 4, 4, 48]    one tile: no neighbour on any axis;
  [2, 32, 8, 8, 96]    seams on all three axes (corner voxels summed from eight slots), two batch items;
  [1, 32, 6, 10, 52]   partial tiles on every axis; the second column tile is four columns wide (one thread per row, with a left
                       neighbour and no right one).
Each with no residual, a residual into level 1, non-zero biases, and both.

Stacked up-sampling: one ``trilinear_ac_soft_argmin`` call on [3 * 2, 4, 6, 8] -> (16, 24, 32) against three calls on its parts
(the aggregator does not take that form: one launch over the stack lost its A/B on the step, docs/design/20; the property stays
pinned because the chain's stacked output invites it).

Aggregator: the eval forward of ``PSMAggregator`` against the same module with ``chain_heads = False`` (one fused-head call per
level), eager and replayed from a graph, at [1, 64, 8, 16, 48] -- where the 32 -> 32 launch does not pick
the head's tile, so both take the two-launch branches: the switch must not change that path -- and at [1, 64, 32, 64, 96], the
smallest volume of these widths at which it does pick it on 256 CUs: there the trunk must hand the three levels over as ONE buffer."""
import pytest
import torch

from densematchingbenchmark_amd import ops, ops_head
from densematchingbenchmark_amd.graph_runner import GraphedForward
from densematchingbenchmark_amd.modeling.stereo.cost_processors.aggregators.PSMNet import PSMAggregator

pytestmark = pytest.mark.gpu

SHAPES = {"one_tile": (1, 32, 4, 4, 48), "seams_b2": (2, 32, 8, 8, 96), "partial": (1, 32, 6, 10, 52)}
RESIDUALS = {"none": (False, False), "res": (True, False), "bias": (False, True), "res_bias": (True, True)}
BIASES = (0.5, -0.25, 0.125)

_levels = {}


def _level_operands(name, dev):
    """Three levels of (x, packed 32 -> 32 weights, packed head weights, scale, shift) and a residual per shape, built once."""
    if name not in _levels:
        shape = SHAPES[name]
        g = torch.Generator().manual_seed(sum(shape))
        lv = []
        for _ in range(3):
            x = torch.randn(shape, generator=g)
            w = torch.randn((32, shape[1], 3, 3, 3), generator=g) / (shape[1] * 27) ** 0.5
            wh = torch.randn((1, 32, 3, 3, 3), generator=g) / (32 * 27) ** 0.5 * 4.0
            scale, shift = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.2
            lv.append((x.to(dev), ops.pack_conv3d_weights(w.to(dev)), ops_head.pack_conv3d_head_weights(wh.to(dev)), scale.to(dev), shift.to(dev)))
        res = torch.randn((shape[0], 1) + shape[2:], generator=g).to(dev)
        _levels[name] = (lv, res)
    return _levels[name]


@pytest.mark.parametrize("case", list(RESIDUALS))
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_chain_finish_equals_the_heads_one_after_the_other(dev, name, n, case):
    with_res, with_bias = RESIDUALS[case]
    lv, res = _level_operands(name, dev)
    B, _, D, H, W = SHAPES[name]
    biases = [b if with_bias else 0.0 for b in BIASES[:n]]
    want, prev = [], res if with_res else None
    for (x, wp, hp, scale, shift), b in zip(lv[:n], biases):
        prev = ops_head.conv3d_k3_head(x, wp, hp, scale, shift, b, prev, True)
        want.append(prev)
    wss = [ops_head.conv3d_k3_head_partial(x, wp, hp, scale, shift, True) for x, wp, hp, scale, shift in lv[:n]]
    got = ops_head.conv3d_head_chain_finish(wss, biases, (B, D, H, W), res if with_res else None)
    assert tuple(got.shape) == (n, B, 1, D, H, W) and bool(torch.isfinite(got).all())
    for k in range(n):
        assert torch.equal(got[k], want[k]), "level %d differs in %d voxels" % (k + 1, int((got[k] != want[k]).sum()))


def test_chain_finish_refuses_what_it_cannot_index(dev):
    from densematchingbenchmark_amd._lib import DmbLibraryError
    lv, _ = _level_operands("one_tile", dev)
    x, wp, hp, scale, shift = lv[0]
    ws = ops_head.conv3d_k3_head_partial(x, wp, hp, scale, shift, True)
    with pytest.raises((DmbLibraryError, RuntimeError)):
        ops_head.conv3d_head_chain_finish([ws] * 5, [0.0] * 5, (1, 4, 4, 48))       # more than four levels
    with pytest.raises((DmbLibraryError, RuntimeError)):
        ops_head.conv3d_head_chain_finish([ws], [0.0], (1, 8, 4, 48))               # a workspace of another shape
    with pytest.raises((DmbLibraryError, RuntimeError)):
        ops_head.conv3d_head_chain_finish([ws[:1000]], [0.0], (1, 4, 4, 46))        # rows that are not 16 bytes


def test_one_upsampling_call_on_the_stack_equals_three(dev):
    B, size = 2, (16, 24, 32)
    x = torch.randn((3 * B, 4, 6, 8), generator=torch.Generator().manual_seed(11)).to(dev) * 3.0
    vals = ops.disp_sample_values(size[0], 0, 1)
    cost, disp = ops.trilinear_ac_soft_argmin(x, size, vals, 1.0)
    assert tuple(cost.shape) == (3 * B,) + size and tuple(disp.shape) == (3 * B, 1) + size[1:]
    for k in range(3):
        c, d = ops.trilinear_ac_soft_argmin(x[k * B:(k + 1) * B], size, vals, 1.0)
        assert torch.equal(cost[k * B:(k + 1) * B], c) and torch.equal(disp[k * B:(k + 1) * B], d)


@pytest.fixture
def no_branch_overlap():
    """Volumes this small take the two-stream form of the forward by default; the chain belongs to the one-stream form."""
    ops.set_branch_overlap(False)
    yield
    ops.set_branch_overlap("auto")


def _aggregator(dev, md):
    from densematchingbenchmark_amd import synthetic
    agg = PSMAggregator(md, in_planes=64).eval()
    synthetic.init_params_(agg, seed=3, classif_gain=10.0)
    return agg.to(dev)


@pytest.mark.parametrize("shape, chained", [((1, 64, 8, 16, 48), False), ((1, 64, 32, 64, 96), True)], ids=["d8_h16_w48", "d32_h64_w96"])
def test_aggregator_forward_equals_the_forward_without_the_chain(dev, no_branch_overlap, shape, chained):
    agg = _aggregator(dev, shape[2] * 4)
    raw = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(dev)
    assert ops_head.conv3d_k3_head_applicable(raw[:, :32]) == chained
    with torch.no_grad():
        got = agg(raw)
        agg.chain_heads = False
        want = agg(raw)
        agg.chain_heads = True
        replayed = GraphedForward(agg, warmup=1)(raw)
        stack = agg.trunk(raw)
    torch.cuda.synchronize()
    assert torch.is_tensor(stack) == chained       # the chain hands the three levels over as one [3, B, 1, D, H, W] buffer
    for level, (g, w, r) in enumerate(zip(got, want, replayed)):
        assert g.shape == w.shape == (shape[0], shape[2] * 4, shape[3] * 4, shape[4] * 4) and g.is_contiguous()
        assert torch.equal(g, w), "cost %d differs" % level
        assert torch.equal(r, w), "replayed cost %d differs" % level
        vals = ops.disp_sample_values(shape[2] * 4, 0, 1)
        dg, dw, dr = (ops.RegressionHint.lookup(c, vals, 1.0, True) for c in (g, w, r))
        assert dg is not None and dw is not None and dr is not None
        assert torch.equal(dg, dw) and torch.equal(dr, dw), "disparity %d differs" % level
        assert torch.equal(dg, ops.soft_argmin(g, vals, 1.0, True)), "the hint of level %d is not the soft-argmin of its cost" % level
