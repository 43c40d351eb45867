"""The backward of DeepPruner's aggregator, the parts that need no GPU: the pack jobs of the stride-(1, 2, 2) units, the two new
functions' argument checks (before any launch), the modules' own refusals (unchanged), and the golden file
tests/golden/deeppruner_aggregator_bwd.npz against autograd through the restatement of tests/_hw_ref.py on the CPU, bit for bit."""
import numpy as np
import os
import pytest
import torch

from densematchingbenchmark_amd import _lib, ops
from densematchingbenchmark_amd.modeling.stereo.cost_processors.aggregators import DeepPrunerAggregator
from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils import HWHourglass
from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers import FusedConv3d
from tests import _hw_bwd_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "deeppruner_aggregator_bwd.npz")


def test_pack_jobs_of_tuple_strides_match_the_pack_group_buffers():
    """unit_pack_jobs returns, for a tuple stride, the two packs the (1, 2, 2) kernels read: the forward pack of the unit and the
    pack of the OTHER direction's kernel on the same tensor, each of the size that kernel asks for (what _PackGroup allocates)."""
    lib = _lib.load()
    hg = HWHourglass(16)
    for k, (ci, co) in enumerate(((16, 32), (32, 64), (64, 128)), start=1):
        down, up = getattr(hg, "conv%d_a" % k), getattr(hg, "conv%d_d" % k)
        assert down.stride == up.stride == FusedConv3d.HW and not down.transposed and up.transposed
        jobs = ops.unit_pack_jobs(down[0].weight, False, down.stride)
        assert jobs == [(co, ci, ops.PACK_CONV), (ci, co, ops.PACK_DECONV)] == ops.unit_pack_jobs(down[0].weight, False, 2)
        # forward: conv ci -> co; data gradient: the transposed kernel co -> ci reading the tensor as [Ci_t, Co_t] = [co, ci]
        assert ops.packed_floats(*jobs[0][:2]) == lib.dmb_conv3d_packed_floats(co, ci)
        assert ops.packed_floats(*jobs[1][:2]) == lib.dmb_deconv3d_packed_floats(co, ci)
        jobs = ops.unit_pack_jobs(up[0].weight, True, up.stride)          # weight [co, ci]: transposed co -> ci
        assert jobs == [(ci, co, ops.PACK_DECONV), (co, ci, ops.PACK_CONV)] == ops.unit_pack_jobs(up[0].weight, True, 2)
        assert ops.packed_floats(*jobs[0][:2]) == lib.dmb_deconv3d_packed_floats(co, ci)
        assert ops.packed_floats(*jobs[1][:2]) == lib.dmb_conv3d_packed_floats(co, ci)      # data gradient: conv ci -> co
    # the 32 -> 16 stride-1 unit: its data gradient is a 16 -> 32 stride-1 launch on the PACK_DGRAD pack
    unit = DeepPrunerAggregator(21, 16).dres1[1]
    assert (unit.in_planes, unit.out_planes, unit.stride) == (32, 16, 1)
    assert ops.unit_pack_jobs(unit[0].weight, False, 1) == [(16, 32, ops.PACK_CONV), (32, 16, ops.PACK_DGRAD)]


def test_new_functions_refuse_cpu_tensors_and_bad_shapes_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_launch)
    hg, agg = HWHourglass(16), DeepPrunerAggregator(21, 16)
    for mod in (hg, hg.eval(), agg, agg.eval()):
        fn, planes = (train_fn.hw_hourglass, 16) if mod is hg else (train_fn.deeppruner_aggregator, 21)
        for shape in ((1, planes, 3, 12, 16), (1, planes, 3, 16, 20), (1, planes + 1, 3, 16, 16), (planes, 3, 16, 16)):
            with pytest.raises(ValueError, match="multiples of 8"):
                fn(mod, torch.zeros(shape))
        with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
            fn(mod, torch.zeros((1, planes, 2, 8, 8)))
        with pytest.raises(_lib.DmbLibraryError, match="no CPU fallback"):
            fn(mod, torch.zeros((1, planes, 2, 8, 8), requires_grad=True))
    with pytest.raises(ValueError, match="skip shape"):
        train_fn.hw_hourglass(hg, torch.zeros((1, 16, 2, 8, 8)), skip=torch.zeros((1, 16, 2, 8, 16)))


def test_data_gradient_wrappers_name_their_channel_sets(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the library was reached")))
    with pytest.raises(_lib.DmbLibraryError, match=r"16 \| 32 \| 64"):
        ops.conv3d_k3_dgrad(torch.zeros((1, 32, 2, 4, 4)), torch.zeros((32, 48, 3, 3, 3)), stride=(1, 2, 2))
    with pytest.raises(_lib.DmbLibraryError, match=r"32 \| 64 \| 128"):
        ops.deconv3d_k3s2_dgrad(torch.zeros((1, 16, 2, 8, 8)), torch.zeros((48, 16, 3, 3, 3)), stride=(1, 2, 2))
    with pytest.raises(_lib.DmbLibraryError, match="does not belong"):
        ops.conv3d_k3_dgrad(torch.zeros((1, 32, 2, 4, 4)), torch.zeros((32, 16, 3, 3, 3)), stride=(1, 2, 2), in_size=(2, 6, 8))
    with pytest.raises(_lib.DmbLibraryError, match="stride"):
        ops.deconv3d_k3s2_dgrad(torch.zeros((1, 16, 2, 8, 8)), torch.zeros((32, 16, 3, 3, 3)), stride=(2, 1, 1))


def test_module_refusals_are_still_in_place():
    x = torch.zeros((1, 16, 2, 8, 8))
    hg = HWHourglass(16).eval()
    with pytest.raises(NotImplementedError, match="no backward"):
        hg(x.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="no backward"):
        HWHourglass(16).train()(x)
    agg = DeepPrunerAggregator(21, 16).eval()
    with pytest.raises(NotImplementedError, match="no backward"):
        agg(torch.zeros((1, 21, 2, 8, 8)))              # eval(), but grad mode on and the parameters require grad
    with pytest.raises(NotImplementedError, match="no backward"):
        with torch.no_grad():
            agg.train()(torch.zeros((1, 21, 2, 8, 8)))
    for unit in (hg.conv1_a, hg.conv1_d, agg.dres1[1]):
        with pytest.raises(NotImplementedError, match="no backward"):
            unit(torch.zeros((1, unit.in_planes, 2, 8, 8)))
    from densematchingbenchmark_amd.modeling.stereo.cost_processors import PROCESSORS
    assert not any("pruner" in k.lower() for k in PROCESSORS)


@pytest.mark.parametrize("name,mode", Q.RUNS, ids=["%s-%s" % r for r in Q.RUNS])
def test_golden_file_is_reproduced_by_the_restatement_bit_for_bit(name, mode):
    z = np.load(GOLDEN)
    res = Q.reference(name, mode, torch.float32)
    prefix = "%s/%s/" % (name, mode)
    assert len(res["grads"]) + 1 == Q.N_TENSORS[Q.CASES[name][0]]
    assert np.array_equal(z[prefix + "loss"], res["loss"].numpy())
    dx = res["dx"]
    if (name, mode) in Q.SAMPLED_DX:
        assert np.array_equal(z[prefix + "dx_samples"], dx.flatten()[Q.positions(prefix + "dx", dx.numel(), Q.SAMPLES_DX)].numpy())
        assert np.array_equal(z[prefix + "dx_stats"], np.array([dx.double().sum().item(), dx.abs().max().item()]))
    else:
        assert np.array_equal(z[prefix + "dx"], dx.numpy())
    for k, g in res["grads"].items():
        assert np.array_equal(z[prefix + "p/" + k + "/samples"], g.flatten()[Q.positions(prefix + k, g.numel())].numpy()), k
        assert np.array_equal(z[prefix + "p/" + k + "/stats"], np.array([g.double().sum().item(), g.abs().max().item()])), k
    buffers = [k for k in z.files if k.startswith(prefix + "b/")]
    assert len(buffers) == (len(res["buffers"]) if mode == "train" else 0)
    for k in buffers:
        assert np.array_equal(z[k], res["buffers"][k[len(prefix) + 2:]].numpy()), k


def test_the_fp32_restatement_meets_the_whole_network_rule_at_these_seeds():
    for name, mode in Q.RUNS:
        r32, r64 = Q.reference(name, mode, torch.float32), Q.reference(name, mode, torch.float64)
        n, tight = Q.whole_network_rule(Q.tensors(r32), Q.tensors(r64), Q.tensors(r32), "%s %s" % (name, mode))
        assert n == tight == Q.N_TENSORS[Q.CASES[name][0]]
