"""The memory contract of tests/test_memory_contract_gpu.py (guarded, poisoned buffers; operands untouched; results bit-identical
to the plain run; 4-byte aligned operands) for the three kernel forms of csrc/conv3d_hw.hip, reached through ``ops.conv3d_k3`` and
``ops.deconv3d_k3s2``.  The cases are built here and run by that module's ``_run_case``; its own table is not touched.

Shapes: a width with W % 4 in {1, 3}, an extent of 1, B = 2 with channel counts off the chunk size (8), and one that spans several
tiles with a partial last one; each with and without a residual."""
import pytest

from tests.test_memory_contract_gpu import Case, Ctx, _run_case, _w3  # noqa: F401  (Ctx: the type a body receives)

pytestmark = pytest.mark.gpu
HW = (1, 2, 2)


def _conv_hw(ops, c, shape, Co, relu, use_res, stride):
    B, Ci, D, H, W = shape
    wp = ops.pack_conv3d_weights(_w3(c, Co, Ci))
    sc, sh = c.affine(Co)
    s = 2 if stride == HW else 1
    oshape = (B, Co, D, (H - 1) // s + 1, (W - 1) // s + 1)
    res = c.t(oshape) if use_res else None
    out = c.out(oshape)
    x = c.t(shape)
    y = ops.conv3d_k3(x, wp, Co, sc, sh, res, stride, relu)
    ops.conv3d_k3(x, wp, Co, sc, sh, res, stride, relu, out=out)
    return [y, out]


def _deconv_hw(ops, c, shape, Co, relu, use_res, stride):
    B, Ci, D, H, W = shape
    wp = ops.pack_deconv3d_weights(_w3(c, Co, Ci, True))
    sc, sh = c.affine(Co)
    oshape = (B, Co, D, 2 * H, 2 * W)
    res = c.t(oshape) if use_res else None
    out = c.out(oshape)
    x = c.t(shape)
    y = ops.deconv3d_k3s2(x, wp, Co, sc, sh, res, relu, stride=stride)
    ops.deconv3d_k3s2(x, wp, Co, sc, sh, res, relu, out=out, stride=stride)
    return [y, out]


_SHAPES = {
    "conv3d_s122": ("conv3d_k3", _conv_hw, HW, {
        "w13_b2_ci5": ((2, 5, 3, 5, 13), 32, True), "w7_ci20_co64": ((1, 20, 2, 6, 7), 64, "pre"),
        "d1h1_w22_ci33_co128": ((1, 33, 1, 1, 22), 128, False), "w1_co16": ((1, 8, 2, 3, 1), 16, True),
        "tiles_h17_w70": ((1, 16, 5, 17, 70), 32, True)}),
    "conv3d_s1_co16": ("conv3d_k3", _conv_hw, 1, {
        "w13_b2_ci5": ((2, 5, 3, 5, 13), 16, True), "w7_ci33": ((1, 33, 2, 3, 7), 16, "pre"),
        "d1h1_w22": ((1, 32, 1, 1, 22), 16, False), "tiles_h9_w70": ((1, 8, 5, 9, 70), 16, True)}),
    "deconv3d_s122": ("deconv3d_k3s2", _deconv_hw, HW, {
        "w13_b2_ci9": ((2, 9, 2, 3, 13), 64, True), "w7_ci20_co16": ((1, 20, 3, 2, 7), 16, "pre"),
        "d1h1_w5": ((1, 16, 1, 1, 5), 32, False), "w1_ci128": ((1, 128, 2, 2, 1), 64, True),
        "tiles_h7_w35": ((2, 33, 5, 7, 35), 32, True)}),
}

CASES = []
for _family, (_wrapper, _body, _stride, _calls) in _SHAPES.items():
    for _label, (_shape, _Co, _relu) in _calls.items():
        for _use_res in (True, False):
            CASES.append(Case(_wrapper, _family, "%s_%s_%s" % (_family, _label, "res" if _use_res else "nores"), _body,
                              (_shape, _Co, _relu, _use_res, _stride), "ok", False))


@pytest.mark.parametrize("case", [pytest.param(k, id=k.id) for k in CASES])
def test_memory_contract(dev, case):
    _run_case(case, dev)
