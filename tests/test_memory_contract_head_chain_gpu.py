"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; no unwritten output
word; results bit-identical to the plain run) for the two halves of the fused classifier tail as calls of their own:
``ops_head.conv3d_k3_head_partial`` (dmb_conv3d_k3_head_partial_f32: the convolution launch, which must overwrite its whole
workspace -- the workspace is the returned tensor here, so a slot word it leaves unwritten keeps the body pattern and fails) and
``ops_head.conv3d_head_chain_finish`` (dmb_conv3d_head_chain_finish_f32: one finishing pass over 1 .. 4 workspaces).  The cases are
built here and run by that module's ``_run_case`` (both poison kinds); that module's own table is not touched.

With the frame in effect the workspaces and the stacked output lie between guards with poisoned bodies: a 16-byte slot read that
starts one column early or ends one late picks up a neighbouring row's sums (the result differs from the plain run only if it is
poison, so the last slot's end = the workspace's end is in every shape), a store past a level's part of the stack lands in the
next level or the guard.  Shapes: one tile; two tiles per axis with batch 2; partial tiles on every axis (W = 52: the second
column tile is four columns wide, its only thread per row has a left neighbour and no right one); one row of four voxels.
The first half refuses an input that is only 4-byte aligned (the kernel needs 16-byte rows).  The chain finish takes a 4-byte
aligned residual on its dword path: its case hands the convolutions an aligned copy of the input and the finish the misaligned
residual."""
import pytest
import torch

from densematchingbenchmark_amd import ops_head
from tests.test_memory_contract_gpu import Case, Ctx, _run_case  # noqa: F401  (Ctx: the type a body receives)

pytestmark = pytest.mark.gpu


def _operands(ops, c, shape, levels, aligned):
    B, Ci, D, H, W = shape
    out = []
    for _ in range(levels):
        x = c.t(shape)
        w = c.t((32, Ci, 3, 3, 3), 1.0 / (Ci * 27) ** 0.5)
        wh = c.t((1, 32, 3, 3, 3), 1.0 / (32 * 27) ** 0.5)
        scale, shift = c.affine(32)
        if aligned and c.misalign:      # the convolution is not the call under test there: it gets 16-byte rows
            x, w, wh, scale, shift = x.clone(), w.clone(), wh.clone(), scale.clone(), shift.clone()
        out.append((x, ops.pack_conv3d_weights(w), ops_head.pack_conv3d_head_weights(wh), scale, shift))
    return out


def _partial(ops, c, shape, relu):
    (x, wp, hp, scale, shift), = _operands(ops, c, shape, 1, False)
    return [ops_head.conv3d_k3_head_partial(x, wp, hp, scale, shift, relu)]


def _chain(ops, c, shape, levels, with_res):
    B, Ci, D, H, W = shape
    wss = [ops_head.conv3d_k3_head_partial(x, wp, hp, scale, shift, True) for x, wp, hp, scale, shift in _operands(ops, c, shape, levels, True)]
    res = c.t((B, 1, D, H, W)) if with_res else None
    y = ops_head.conv3d_head_chain_finish(wss, [0.5, -0.25, 0.125, 1.0][:levels], (B, D, H, W), res)
    return [y] + wss


_SHAPES = {
    "conv3d_k3_head_partial": (_partial, "refuse", {"one_tile": ((1, 32, 4, 4, 48), True), "seams_b2_w96": ((2, 32, 8, 8, 96), True),
                                                    "partial_w52": ((1, 32, 6, 10, 52), True), "ci3_d1_h1_w4": ((2, 3, 1, 1, 4), False)}),
    "conv3d_head_chain_finish": (_chain, "ok", {"one_tile_n1": ((1, 32, 4, 4, 48), 1, False), "seams_b2_w96_n3_res": ((2, 32, 8, 8, 96), 3, True),
                                                "partial_w52_n2_res": ((1, 32, 6, 10, 52), 2, True), "partial_w52_n4": ((1, 8, 6, 10, 52), 4, False),
                                                "d1_h1_w4_n3_res": ((2, 3, 1, 1, 4), 3, True)}),
}

CASES = [Case(_wrapper, "head_chain", _label, _body, _args, _misalign, False)
         for _wrapper, (_body, _misalign, _calls) in _SHAPES.items() for _label, _args in _calls.items()]


@pytest.mark.parametrize("case", [pytest.param(k, id=k.id) for k in CASES])
def test_memory_contract(dev, case):
    _run_case(case, dev)
