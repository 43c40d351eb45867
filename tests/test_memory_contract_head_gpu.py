"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; no unwritten output
word; results bit-identical to the plain run) for the two launching wrappers of ``ops_head``: ``pack_conv3d_head_weights``
(dmb_conv3d_head_pack_weights_f32) and ``conv3d_k3_head`` (dmb_conv3d_k3_head_f32: the convolution launch that leaves its partial
sums in the workspace, and the finishing pass).  The cases are built here and run by that module's ``_run_case`` (both poison
kinds); that module's own table is not touched.

With the frame in effect the wrapper's output AND its workspace lie between guards with poisoned bodies: a partial-sum tile
written past its slot, a slot never written but read by the finishing pass (poison reaches the result: NaN, or 1e30-sized values
that differ from the plain run's) and a store past the output all show.  Shapes: one tile (all halo sums dropped); two tiles per
axis; partial tiles in z, y and x with batch 2 (the last slot's end is the workspace's end) and the residual; an input with
fewer channels than a chunk pair.  Operands that are only 4-byte aligned are refused (the kernel needs 16-byte rows)."""
import pytest
import torch

from densematchingbenchmark_amd import ops_head
from tests.test_memory_contract_gpu import Case, Ctx, _run_case  # noqa: F401  (Ctx: the type a body receives)

pytestmark = pytest.mark.gpu


def _pack(ops, c, scale):
    return [ops_head.pack_conv3d_head_weights(c.t((1, 32, 3, 3, 3), scale))]


def _head(ops, c, shape, with_res, relu):
    B, Ci, D, H, W = shape
    x = c.t(shape)
    w = c.t((32, Ci, 3, 3, 3), 1.0 / (Ci * 27) ** 0.5)
    wh = c.t((1, 32, 3, 3, 3), 1.0 / (32 * 27) ** 0.5)
    scale, shift = c.affine(32)
    res = c.t((B, 1, D, H, W)) if with_res else None
    wp, hp = ops.pack_conv3d_weights(w), ops_head.pack_conv3d_head_weights(wh)
    return [ops_head.conv3d_k3_head(x, wp, hp, scale, shift, 0.5, res, relu), hp]


_SHAPES = {
    "pack_conv3d_head_weights": (_pack, {"unit": (1.0,), "small": (0.05,)}),
    "conv3d_k3_head": (_head, {"one_tile": ((1, 32, 4, 4, 48), False, True), "seams_w96": ((1, 32, 8, 8, 96), False, True),
                               "partial_b2_w52_res": ((2, 32, 5, 6, 52), True, True), "ci3_d1_h1_w4": ((2, 3, 1, 1, 4), True, False)}),
}

CASES = [Case(_wrapper, "head", _label, _body, _args, "refuse" if _wrapper == "conv3d_k3_head" else "ok", False)
         for _wrapper, (_body, _calls) in _SHAPES.items() for _label, _args in _calls.items()]


@pytest.mark.parametrize("case", [pytest.param(k, id=k.id) for k in CASES])
def test_memory_contract(dev, case):
    _run_case(case, dev)
