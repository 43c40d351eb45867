"""The DeepPruner training losses on the CPU: reached by import, ``DeepPrunerLoss`` built from this repository's two config files and
from the reference's two configs, every refusal before a launch, the refusals of the four entry points of csrc/deeppruner_loss.hip
and of their wrappers, the header against the ctypes table, the registries that stay as they were, and the restatement
(tests/_deeppruner_loss_ref.py) against the real reference's recording (tests/golden/deeppruner_loss.npz,
scripts/gen_golden_deeppruner_loss.py), empty masks included."""
import ctypes
import inspect
import json
import os

import pytest
import torch

from densematchingbenchmark_amd import _lib, ops, ops_deeppruner
from densematchingbenchmark_amd.config import Config
from tests import _deeppruner_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = 100001, 100002
RELS = {"4x": "configs/DeepPruner/scene_flow_4x.py", "8x": "configs/DeepPruner/scene_flow_8x.py"}
NEW = ("dmb_deeppruner_loss_fwd_f32", "dmb_deeppruner_loss_bwd_f32", "dmb_quantile_loss_fwd_f32", "dmb_quantile_loss_bwd_f32")


def _reference_settings(rel):
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as fp:
        return json.load(fp)[rel]["settings"]


def _configs(name):
    return Config.fromfile(os.path.join(ROOT, RELS[name])), Config(_reference_settings(RELS[name]))


def test_import_paths_and_signatures():
    from densematchingbenchmark_amd.modeling.stereo import losses
    from densematchingbenchmark_amd.modeling.stereo.losses import DeepPrunerLoss
    from densematchingbenchmark_amd.modeling.stereo.losses.deeppruner_loss import DeepPrunerLoss as direct
    from densematchingbenchmark_amd.modeling.stereo.losses.utils import quantile_loss
    from densematchingbenchmark_amd.modeling.stereo.losses.utils.quantile_loss import quantile_loss as direct_q
    assert DeepPrunerLoss is direct and quantile_loss is direct_q and "DeepPrunerLoss" in losses.__all__
    assert str(inspect.signature(quantile_loss)) == "(minEstDisp, maxEstDisp, gtDisp, max_disp, start_disp=0, weight=1.0, theta=0.05)"
    assert list(inspect.signature(DeepPrunerLoss.__call__).parameters) == ["self", "disps", "min_disparity", "max_disparity", "target"]
    for fn in ("deeppruner_loss_fwd", "deeppruner_loss_bwd", "quantile_loss_fwd", "quantile_loss_bwd"):
        src = inspect.getsource(getattr(ops_deeppruner, fn))
        assert not hasattr(ops, fn) and 'launch("dmb_' in src and "torch.empty(" in src and "empty_like" not in src and "new_empty" not in src
    assert ops_deeppruner.torch is torch


@pytest.mark.parametrize("name", list(RELS))
def test_construction_from_the_shipped_and_the_reference_configs(name):
    from densematchingbenchmark_amd.modeling.stereo.losses import DeepPrunerLoss
    weights, theta = R.CASES[name][4], R.CASES[name][5]
    for cfg in _configs(name):
        loss = DeepPrunerLoss(cfg)
        assert loss.weights == list(weights) and loss.theta == theta and (loss.l1_weight, loss.q_weight) == (1.0, 1.0)
        assert (loss.l1_lower, loss.l1_upper, loss.q_lower, loss.q_upper) == (0.0, 192.0, 0.0, 192.0)
    assert DeepPrunerLoss(Config(R.settings(name))).weights == list(weights)
    shifted = Config(R.settings(name))
    shifted.model.losses.quantile_loss.start_disp = 4
    assert (DeepPrunerLoss(shifted).q_lower, DeepPrunerLoss(shifted).q_upper) == (4.0, 196.0)


def test_refusals_come_before_any_launch(monkeypatch):
    """Every launch goes through ``_lib.load()``: with it replaced by a function that fails the test, a refusal that raises its
    own error has launched nothing."""
    from densematchingbenchmark_amd.modeling.stereo.losses import DeepPrunerLoss
    from densematchingbenchmark_amd.modeling.stereo.losses.utils import quantile_loss

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_launch)
    for node in ("l1_loss", "quantile_loss"):
        cfg = Config(R.settings("4x"))
        del cfg.model.losses[node]
        with pytest.raises(ValueError, match="l1_loss and the quantile_loss"):
            DeepPrunerLoss(cfg)
    sparse = Config(R.settings("4x"))
    sparse.data.sparse = True
    with pytest.raises(NotImplementedError, match="sparse"):
        DeepPrunerLoss(sparse)
    bad_theta = Config(R.settings("4x"))
    bad_theta.model.losses.quantile_loss.theta = 1.5
    with pytest.raises(ValueError, match="theta"):
        DeepPrunerLoss(bad_theta)
    loss = DeepPrunerLoss(Config(R.settings("4x")))                       # four weights: a list of two maps and the two range maps
    disps, lo, hi, gt = R.inputs("8x")                                     # a list of three
    with pytest.raises(ValueError, match="l1 weights"):
        loss(disps, lo, hi, gt)
    with pytest.raises(ValueError, match="l1 weights"):
        loss(disps[:1], lo, hi, gt)
    full = torch.zeros((1, 1, 4, 6))
    with pytest.raises(ValueError, match="theta"):
        quantile_loss(full, full, full, 192, theta=0.0)
    with pytest.raises(ValueError, match="one shape"):
        quantile_loss(full, full, torch.zeros((1, 1, 8, 12)), 192)


def test_cpu_tensors_meet_the_no_cpu_fallback_error():
    from densematchingbenchmark_amd.modeling.stereo.losses import DeepPrunerLoss
    from densematchingbenchmark_amd.modeling.stereo.losses.utils import quantile_loss
    disps, lo, hi, gt = R.inputs("4x")
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        DeepPrunerLoss(Config(R.settings("4x")))(disps, lo, hi, gt)
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        quantile_loss(gt, gt, gt, 192)
    stats, go = torch.zeros((2,), dtype=torch.float64), torch.ones((6,))
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        ops_deeppruner.deeppruner_loss_bwd(disps, lo, hi, gt, stats, go, 0, 192, 0, 192, 0.05)
    with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
        ops_deeppruner.quantile_loss_bwd(gt, gt, gt, stats, go[:2], 0, 192, 0.05)


def test_wrappers_refuse_bad_operands_on_the_host():
    disps, lo, hi, gt = R.inputs("4x")
    ok = (0, 192, 0, 192, 0.05)
    for args in (([], lo, hi, gt) + ok, (disps * 2, lo, hi, gt) + ok, ([disps[0].double()], lo, hi, gt) + ok,
                 (disps, lo.double(), hi, gt) + ok, (disps, lo, hi[:, :, :4], gt) + ok, (disps, lo, hi, gt[0]) + ok,
                 (disps, lo, hi, gt.double()) + ok, (disps, lo, hi, torch.cat((gt, gt))) + ok,
                 ([disps[0][0]], lo, hi, gt) + ok, (disps, lo, hi, gt, 0, 192, 0, 192, 0.0), (disps, lo, hi, gt, 0, 192, 0, 192, 1.0)):
        with pytest.raises(_lib.DmbLibraryError):
            ops_deeppruner.deeppruner_loss_fwd(*args)
    stats = torch.zeros((2,), dtype=torch.float64)
    for bad_stats, bad_go in ((stats.float(), torch.ones((6,))), (torch.zeros((3,), dtype=torch.float64), torch.ones((6,))),
                              (stats, torch.ones((5,))), (stats, torch.ones((6,), dtype=torch.float64))):
        with pytest.raises(_lib.DmbLibraryError):
            ops_deeppruner.deeppruner_loss_bwd(disps, lo, hi, gt, bad_stats, bad_go, *ok)
    for args in ((gt, gt[:, :, :4], gt, 0, 192, 0.05), (gt.double(), gt, gt, 0, 192, 0.05), (gt[0], gt[0], gt[0], 0, 192, 0.05),
                 (gt, gt, gt, 0, 192, 2.0)):
        with pytest.raises(_lib.DmbLibraryError):
            ops_deeppruner.quantile_loss_fwd(*args)
    with pytest.raises(_lib.DmbLibraryError):
        ops_deeppruner.quantile_loss_bwd(gt, gt, gt, stats, torch.ones((3,)), 0, 192, 0.05)


def _fake():
    """A non-NULL host address: the entry point must refuse before any device call, so it is never dereferenced."""
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def test_entry_points_validate_before_any_device_call():
    lib = _lib.load()
    keep, p = _fake()
    sizes = _lib.host_ints([8, 4, 2])
    big = _lib.host_ints([1 << 15, 4, 2])
    bounds = (0.0, 192.0, 0.0, 192.0, 0.05)
    fused = {
        "deeppruner_loss_fwd": (lib.dmb_deeppruner_loss_fwd_f32, ("d0", "d1", "d2", "hs", "ws", "lo", "hi", "gt", "ws64", "out", "stats")),
        "deeppruner_loss_bwd": (lib.dmb_deeppruner_loss_bwd_f32, ("d0", "d1", "d2", "hs", "ws", "lo", "hi", "gt", "stats", "go", "g0", "g1",
                                                                  "g2", "glo", "ghi")),
    }
    for who, (fn, pointers) in fused.items():
        names = pointers + ("K", "B", "h", "w", "H", "W", "l1_lo", "l1_hi", "q_lo", "q_hi", "theta")
        ok = dict(zip(names, tuple(sizes if n in ("hs", "ws") else p for n in pointers) + (3, 1, 2, 2, 8, 8) + bounds))

        def call(**change):
            args = dict(ok)
            args.update(change)
            return fn(*[args[n] for n in names], None)

        changes = [(dict([(n, None)]), EINVAL) for n in pointers]
        changes += [(dict(B=0), EINVAL), (dict(h=0), EINVAL), (dict(w=-1), EINVAL), (dict(H=0), EINVAL), (dict(W=-8), EINVAL),
                    (dict(hs=_lib.host_ints([8, 0, 2])), EINVAL), (dict(ws=_lib.host_ints([8, 4, -2])), EINVAL),
                    (dict(theta=0.0), EINVAL), (dict(theta=1.0), EINVAL), (dict(theta=-0.5), EINVAL), (dict(theta=float("nan")), EINVAL),
                    (dict(K=0), EUNSUPPORTED), (dict(K=4), EUNSUPPORTED), (dict(K=-1), EUNSUPPORTED),
                    (dict(H=1 << 15, W=1 << 14), EUNSUPPORTED),                      # a 2 GiB ground-truth item
                    (dict(h=1 << 15, w=1 << 14), EUNSUPPORTED),                      # a 2 GiB range map
                    (dict(hs=big, ws=_lib.host_ints([1 << 14, 4, 2])), EUNSUPPORTED)]   # a 2 GiB list map
        for change, code in changes:
            assert call(**change) == code, (who, change)
            assert who.encode() in lib.dmb_last_error(), (who, change)
        # a NULL among the K maps the list holds is refused; beyond K it is not read
        assert call(K=2, d1=None) == EINVAL and call(K=1, d0=None) == EINVAL
        if who.endswith("bwd"):
            assert call(K=2, g1=None) == EINVAL and who.encode() in lib.dmb_last_error()
    plain = {
        "quantile_loss_fwd": (lib.dmb_quantile_loss_fwd_f32, ("lo", "hi", "gt", "ws64", "out", "stats")),
        "quantile_loss_bwd": (lib.dmb_quantile_loss_bwd_f32, ("lo", "hi", "gt", "stats", "go", "glo", "ghi")),
    }
    for who, (fn, pointers) in plain.items():
        names = pointers + ("B", "H", "W", "q_lo", "q_hi", "theta")
        ok = dict(zip(names, (p,) * len(pointers) + (1, 8, 8, 0.0, 192.0, 0.05)))
        changes = [(dict([(n, None)]), EINVAL) for n in pointers]
        changes += [(dict(B=0), EINVAL), (dict(H=-1), EINVAL), (dict(W=0), EINVAL), (dict(theta=0.0), EINVAL), (dict(theta=1.5), EINVAL),
                    (dict(H=1 << 15, W=1 << 14), EUNSUPPORTED)]
        for change, code in changes:
            args = dict(ok)
            args.update(change)
            assert fn(*[args[n] for n in names], None) == code, (who, change)
            assert who.encode() in lib.dmb_last_error(), (who, change)
    del keep


def test_header_table_abi_and_registries():
    from densematchingbenchmark_amd.modeling import build_model
    from densematchingbenchmark_amd.modeling.stereo import models
    from densematchingbenchmark_amd.modeling.stereo.cost_processors import PROCESSORS
    from densematchingbenchmark_amd.modeling.stereo.losses import builder, make_gsm_loss_evaluator
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES) and all(n in _lib.SIGNATURES for n in NEW)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW) and lib.dmb_abi_version() == _lib.ABI_VERSION
    header = open(_lib.HEADER_PATH).read()
    assert "#define DMB_DEEPPRUNER_LOSS_WORKSPACE_DOUBLES %d\n" % _lib.DEEPPRUNER_LOSS_WORKSPACE_DOUBLES in header
    assert set(PROCESSORS) == {'Difference', 'Concatenation', 'Correlation'}
    assert set(models._META_ARCHITECTURES) == {"GeneralizedStereoModel", "AnyNet"}
    assert set(builder._FACTORIES) == {"l1_loss", "focal_loss"}
    for name in RELS:
        for cfg in _configs(name):
            with pytest.raises(ValueError, match="quantile_loss not implemented"):      # the evaluator of the other models stays as it was
                make_gsm_loss_evaluator(cfg)
            with pytest.raises(NotImplementedError):
                build_model(cfg)


def _close(a, b):
    return abs(a - b) <= 2e-6 * max(1.0, abs(b))


@pytest.mark.parametrize("name", R.RECORDED)
def test_restatement_meets_the_recording(name):
    """Bit for bit on the recording's CPU (the generator asserts it); elsewhere ATen may sum a mean in another order, so each loss is
    held to 2e-6 * max(1, |loss|) and each gradient tensor to 2e-6 of its largest element."""
    z = R.recording()
    K = len(R.CASES[name][1])
    assert [str(k) for k in z[name + "/keys"]] == ["quantile_loss"] + ["l1_loss_lvl%d" % i for i in range(K + 2)]
    fractions = z[name + "/fractions"]
    assert all(0.1 <= f <= 0.9 for f in fractions[:K + 4]) and fractions[K + 5] > 0 and fractions[K + 6] > 0
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        losses, grads = R.run(name, dtype)
        rec = z["%s/loss%s" % (name, tag)]
        exact = all(torch.equal(a, torch.from_numpy(rec)[i]) for i, a in enumerate(losses))
        print("%s fp%s: losses %s the recording" % (name, tag, "equal" if exact else "are close to"))
        assert all(_close(a.item(), float(b)) for a, b in zip(losses, rec)), (name, tag)
        for i, g in enumerate(grads):
            want = torch.from_numpy(z["%s/grad%s_%d" % (name, tag, i)])
            assert g.shape == want.shape and (g - want).abs().max() <= 2e-6 * want.abs().max(), (name, tag, i)


@pytest.mark.parametrize("name", R.RECORDED)
def test_empty_masks_follow_the_reference(name):
    """No valid pixel: every smooth-L1 level is 0, the quantile loss is NaN (the mean of an empty tensor), all gradients are zero."""
    z = R.recording()
    rec = z[name + "/empty_loss32"]
    assert bool(torch.isnan(torch.tensor(rec[0]))) and (rec[1:] == 0).all() and float(z[name + "/empty_grad_max"].max()) == 0.0
    for dtype in (torch.float32, torch.float64):
        losses, grads = R.run(name, dtype, empty=True)
        assert bool(torch.isnan(losses[0])) and all(v.item() == 0.0 for v in losses[1:])
        assert all(int(g.ne(0).sum()) == 0 for g in grads)
