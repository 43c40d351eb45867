"""Host-side facts of the large-tensor table (tests/_large.py), checked without a GPU: the table covers the header, every row
meets the shape conditions its GPU test relies on, and the plan queries accept the planned convolution rows."""
import re

import torch

from tests import _large

ROWS = _large.rows()

# Entry points of include/dmb_hip.h without a row, each with its reason.  A new entry point fails test_table_covers_the_header
# until it has a row or a line here.
_NO_LAUNCH_SIZE = {
    r"dmb_(abi_version|last_error|build_id)": "reports the library, launches nothing",
    r"dmb_\w+_plan": "plan query: host-only, exercised by test_plan_queries_accept_the_planned_rows",
    r"dmb_\w*(packed_floats|packed_bytes|workspace_floats|workspace_doubles|bnstats_partials|head_preferred)": "size query: host-only",
    r"dmb_\w*pack_\w*weights\w*": "weight packer: its operand is one layer's weight, no batch",
}
_NOT_YET = """
dmb_fast_cat_fms_f32 dmb_fast_dif_fms_f32 dmb_fast_fms_bwd_f32 dmb_spn_gaterecurrent2d_f32 dmb_spn_gaterecurrent2d_bwd_f32
dmb_catconv_finalize_f32 dmb_catconv_combine_f32 
dmb_preact_conv_f32
dmb_conf_gather_f32 dmb_conf_phase_conv2d_f32 dmb_conf_ring_f32 dmb_patch_match_step_f32
dmb_deeppruner_volume_f32 
dmb_anynet_final_maps_f32 dmb_deeppruner_final_maps_f32 
dmb_stereo_focal_loss_fwd_f32 dmb_stereo_focal_loss_bwd_f32 dmb_map_loss_fwd_f32 dmb_map_loss_bwd_f32 dmb_conv3d_k3_wgrad_f32
dmb_conv3d_k3s2_wgrad_f32 dmb_conv2d_wgrad_f32 dmb_conv3d_k3_bnstats_f32 dmb_bn_train_act_f32 
dmb_bn_act_bwd_f32 dmb_cat_first_wgrad_maps_f32 

dmb_patch_match_step_bwd_f32 dmb_deeppruner_uniform_samples_bwd_f32
dmb_deeppruner_loss_fwd_f32 dmb_deeppruner_loss_bwd_f32 dmb_quantile_loss_fwd_f32 dmb_quantile_loss_bwd_f32
""".split()
EXCLUDED = {name: _large.NOT_YET_COVERED for name in _NOT_YET}
for _name in ("dmb_spn_gaterecurrent2d_f32", "dmb_spn_gaterecurrent2d_bwd_f32"):
    EXCLUDED[_name] += ": five and ten operands of one shape, 43 GiB and more at 2^31 elements, past the 40 GiB cap of a row"
for _name in ("dmb_conv3d_k3_wgrad_f32", "dmb_conv3d_k3s2_wgrad_f32", "dmb_conv2d_wgrad_f32", "dmb_cat_first_wgrad_maps_f32"):
    EXCLUDED[_name] += ": the dense pass needs an FP32 yardstick for a sum of 7e7 products per weight, which slice launches do not give"

# The entry points with a torch-shim path (csrc/torch_shim.cpp): a covered one runs once through each binding.
SHIM_ENTRIES = ("dmb_conv3d_k3_f32", "dmb_deconv3d_k3s2_f32", "dmb_conv3d_k3_c1_f32", "dmb_conv2d_f32", "dmb_copy_window_f32",
                "dmb_trilinear_ac_soft_argmin_f32", "dmb_conv3d_k3_head_f32", "dmb_conv3d_head_chain_finish_f32", "dmb_bn_train_fwd_f32")

# What dmb_*_plan returns for each planned row at its full batch count (form << 8 | tile, include/dmb_hip.h), 256 compute units,
# single-chain kernels, 16-byte aligned operands.  The FORM is the same at the batch count of every slice of check (b) -- a host-checked
# fact below -- and every form but split-K is one k-ordered fma chain per output whatever the tile, so (b) compares bit for bit.
PLANNED = {
    "conv3d_k3_f32-s1_32to32_res_relu": 0x301, "conv3d_k3_f32-s1_64to64": 0x204, "conv3d_k3_f32-s2_32to64": 0x501,
    "conv3d_k3_f32-s1_20to32": 0x301, "conv3d_k3_f32-s1_32to32_vec": 0x203, "deconv3d_k3s2_f32-queue_64to32": 0x200,
    "deconv3d_k3s2_f32-parity_64to64": 0x305, "conv2d_f32-k3_32to32": 0x200, "conv2d_f32-k1_64to32": 0x211,
    "conv2d_f32-k3_dil4_32to32": 0x20d, "conv2d_f32-k3_windows": 0x204,
}


def _excluded(name):
    if name in EXCLUDED:
        return EXCLUDED[name]
    for pattern, reason in _NO_LAUNCH_SIZE.items():
        if re.fullmatch(pattern, name):
            return reason
    return None


def test_table_covers_the_header():
    """Every entry point the parser of the ctypes table finds in include/dmb_hip.h has a row or an explicit exclusion."""
    from densematchingbenchmark_amd import _lib
    covered = {r.entry for r in ROWS} | {n for r in ROWS for n in r.also}
    assert covered <= set(_lib.PROTOTYPES), sorted(covered - set(_lib.PROTOTYPES))
    missing = [n for n in _lib.PROTOTYPES if n not in covered and _excluded(n) is None]
    assert not missing, "entry points without a large-tensor row or an exclusion: %s" % missing
    both = sorted(n for n in covered if _excluded(n) is not None)
    assert not both, "excluded and covered at once: %s" % both
    stale = sorted(set(EXCLUDED) - set(_lib.PROTOTYPES))
    assert not stale, "exclusions of entry points the header no longer declares: %s" % stale
    # an excluded entry point that launches on a batch, a row count or an element count is only ever "not yet covered"
    sized = {"B", "B2", "N", "rows", "n", "njobs", "nmaps"}
    for name, (_, params) in _lib.PROTOTYPES.items():
        reason = _excluded(name)
        if reason is not None and not reason.startswith(_large.NOT_YET_COVERED) and params and params[-1][1] == "stream":
            assert not sized & {p for _, p in params} or "pack" in name, (name, reason)
    for name in SHIM_ENTRIES:
        assert {r.binding for r in ROWS if r.entry == name} == {"ctypes", "shim"}, name
    assert len({r.id for r in ROWS}) == len(ROWS)


def test_every_row_meets_the_shape_conditions():
    for r in ROWS:
        E = 1
        for v in r.items[r.large]:
            E *= v
        assert r.B * E > 1 << 31, r.id                                   # more than 2^31 elements, so more than 8 GiB
        ib = r.item_bytes(r.large)
        assert ib == 4 * E, r.id                                         # (the large operand is FP32 in every row)
        for line in _large.LINES:
            assert line % ib != 0 and line < r.B * ib, (r.id, line)      # each byte line strictly inside an item
        idx = r.checked_items()
        assert len(idx) <= 8 and idx[0] == 0 and idx[-1] == r.B - 1, r.id
        for line in _large.LINES:
            assert line // ib in idx and line // ib + 1 in idx, (r.id, line)
        assert all(r.item_bytes(n) < _large.ITEM_LIMIT_BYTES for n in r.items), r.id       # far below every per-item limit
        assert r.B <= _large.GRID_LIMIT, r.id
        sl = r.slices()
        assert sl[0][0] == 0 and sl[-1][1] == r.B and all(a[1] == b[0] for a, b in zip(sl, sl[1:])), r.id
        assert all((b1 - b0) * r.item_bytes(n) < 1 << 31 for b0, b1 in sl for n in r.items), r.id
        assert r.peak_bytes() <= _large.PEAK_CAP_BYTES, (r.id, r.peak_bytes())
        assert r.kind in ("item", "reduce") and r.family in (1, 2, 3, 4), r.id
        assert set(r.inputs) <= set(r.items) and (r.outputs or r.reduced) and r.large in r.items, r.id
        assert all(r.dtypes.get(n, torch.float32) in (torch.float32, torch.uint8) for n in r.inputs), r.id


def test_plan_queries_accept_the_planned_rows():
    from densematchingbenchmark_amd import _lib
    lib = _lib.load()
    seen = {}
    for r in ROWS:
        if r.plan is None:
            continue
        assert all(r.item_bytes(n) % 16 == 0 for n in r.items), r.id      # a slice's operands are 16-byte aligned like the whole's
        code = _large.plan_code(lib, r.plan, r.B)
        assert code > 0, "%s: refused with %d (%s)" % (r.id, code, lib.dmb_last_error().decode())
        key = r.id[:-len(r.binding) - 1] if r.binding else r.id
        seen[key] = code
        for b0, b1 in r.slices():
            part = _large.plan_code(lib, r.plan, b1 - b0)
            assert part > 0 and part >> 8 == code >> 8, "%s: form 0x%x at B = %d, 0x%x at %d" % (r.id, code, r.B, part, b1 - b0)
        assert code >> 8 != 1, "%s: split-K under single_chain" % r.id
    print({k: hex(v) for k, v in seen.items()})
    assert seen == PLANNED


def test_references_run_in_both_precisions():
    """Each item-wise row's reference on two random items, in FP64 and in FP32: the shapes of the table, finite values, and an FP32
    evaluation that stays within FP32 rounding of the FP64 one (the yardstick of check (a) is not itself broken)."""
    for r in ROWS:
        if r.kind != "item":
            continue
        g = torch.Generator().manual_seed(11)
        t = {n: (torch.randint(0, 256, (2,) + tuple(r.items[n]), generator=g, dtype=torch.uint8) if r.dtypes.get(n) == torch.uint8 else
                 torch.randn((2,) + tuple(r.items[n]), generator=g) * r.scale.get(n, 1.0) + r.mean.get(n, 0.0)) for n in r.inputs}
        shared = r.shared(3)
        r64 = getattr(r, "ref64", r.ref)(_large._cast(t, torch.float64), _large._cast(shared, torch.float64))
        r32 = r.ref(t, shared)
        assert len(r64) == len(r32) == len(r.outputs), r.id
        for n, a, b in zip(r.outputs, r64, r32):
            assert tuple(a.shape) == tuple(b.shape) == (2,) + tuple(r.items[n]), (r.id, n, tuple(a.shape))
            assert bool(torch.isfinite(a.double()).all()) and bool(torch.isfinite(b.double()).all()), (r.id, n)
            if n not in r.exact:
                assert a.dtype == torch.float64 and b.dtype == torch.float32, (r.id, n)
                assert (a - b.double()).abs().max().item() <= 1e-4 * max(1.0, a.abs().max().item()), (r.id, n)
