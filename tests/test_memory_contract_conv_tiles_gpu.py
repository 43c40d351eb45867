"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; every output word
written; results bit-identical to the plain run) for EVERY tile instantiation ``ops.conv3d_k3`` can plan for a full-grid launch, and
for ``ops.conv3d_k3_bnstats`` on the three larger 32-channel tiles.

That module's table runs tiny edge shapes (at most about 2e5 output elements), and a launch that small takes the smallest tile of
each list or split-K (csrc/conv3d_s1s2.hip picks by workgroup rounds): the partial-tile zero fill and epilogue masks of the larger
tiles never ran between guard pages.  Here: one launch per plan code from GPU_CASES of tests/test_conv3d_plan_host.py -- the
smallest shape that reaches the code with a partial last tile along every axis of that tile, B = 2 so that the last item's end is
the operand's end -- with folded affine, skip operand and ReLU, into a fresh tensor and into the caller's ``out=``; plain, inside
``Frame("nan")`` and inside ``Frame("huge")``, rules (a) - (e) of that module through its ``_check_framed``.  Each body first asserts
that the launch it is about to make has the recorded plan on this device.  The existing module's table and its size rule stay as
they are; these shapes exceed it, which is why they live here."""
import pytest
import torch

from tests._framed import PATTERNS
from tests.test_conv3d_plan_host import GPU_CASES, TILES
from tests.test_memory_contract_gpu import Case, Ctx, _check_framed, _execute, _snapshot, _w3  # noqa: F401  (Ctx: the type a body receives)

pytestmark = pytest.mark.gpu


def _out(c, shape, shift):
    """``c.out(shape)``; with ``shift`` the body starts 4 bytes off the 16-byte alignment while every other operand stays aligned."""
    if not shift:
        return c.out(shape)
    c.outs += 1
    if c.frame is not None:
        return c.frame.alloc(shape, torch.float32, c.dev, "poison", misalign=4)
    n = 1
    for s in shape:
        n *= int(s)
    d = torch.empty(n + 1, dtype=torch.float32, device=c.dev)[1:].view(shape)
    d.view(-1).view(torch.int32).fill_(PATTERNS["nan"][1])
    return d


def _conv_tile(ops, c, Ci, Co, stride, shape, code, shift):
    B, D, H, W = shape
    wp = ops.pack_conv3d_weights(_w3(c, Co, Ci))
    sc, sh = c.affine(Co)
    oshape = (B, Co) + tuple((e - 1) // stride + 1 for e in (D, H, W))
    res = c.t(oshape)
    out = _out(c, oshape, shift)
    x = c.t((B, Ci, D, H, W))
    assert ops.conv3d_k3_plan(x, Co, stride, res, out) == code, "this device plans another instantiation than the case was recorded for"
    ops.conv3d_k3(x, wp, Co, sc, sh, res, stride, True, out=out)
    if shift:      # (a fresh output is 16-byte aligned: another plan)
        return [out]
    assert ops.conv3d_k3_plan(x, Co, stride, res) == code
    return [ops.conv3d_k3(x, wp, Co, sc, sh, res, stride, True), out]


def _bnstats_tile(ops, c, Ci, shape, code):
    B, D, H, W = shape
    x = c.t((B, Ci, D, H, W))
    before = ops.split_k()
    ops.set_split_k(False)      # (the statistics launch follows the single-chain pick)
    try:
        assert ops.conv3d_k3_plan(x, 32) == code
    finally:
        ops.set_split_k(before)
    fused = ops.conv3d_k3_bnstats(x, ops.pack_conv3d_weights(_w3(c, 32, Ci)), 32)
    assert fused is not None, "the epilogue form is expected to cover this shape"
    tx, ty, tz = TILES[code]
    assert fused[1].shape[1] == B * -(-W // tx) * -(-H // ty) * -(-D // tz)
    return list(fused)


CASES = [Case("conv3d_k3", "conv3d_tiles", "%s_plan_%03x" % (name, code), _conv_tile, (Ci, Co, stride, shape, code, shift), "ok", False)
         for name, Ci, Co, stride, shape, code, _, shift in GPU_CASES]
CASES += [Case("conv3d_k3_bnstats", "conv3d_tiles", "%s_plan_%03x" % (name, code), _bnstats_tile, (Ci, shape, code), "declines", False)
          for name, Ci, Co, stride, shape, code, _, shift in GPU_CASES if code in (0x200, 0x201, 0x202)]


@pytest.mark.parametrize("case", [pytest.param(k, id=k.id) for k in CASES])
def test_memory_contract(dev, case):
    c, res = _execute(case, dev)
    plain = _snapshot(c, res)
    for kind in ("nan", "huge"):
        _check_framed(case, dev, kind, 0, plain)
