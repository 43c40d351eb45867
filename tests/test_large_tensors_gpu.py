"""Every kernel on an operand of more than 2^31 elements: byte offsets past 2 GiB (an ``int`` byte offset wraps), past 4 GiB (an
``unsigned`` one) and element indices past 2^31 (``int off = b * C * HW``; a Python int cut by a ``c_int`` or an ``(int)`` cast).

tests/_large.py holds the table -- one row per entry point and binding -- and the harness.  The size comes from the batch count:
every item is a small awkward shape far below the per-item limits (include/dmb_hip.h, "Sizes"), so what is exercised is the 64-bit
base ACROSS items, which no other test launches.  An item-wise row is checked (a) against the plain FP64 / FP32 reference at item 0,
item B - 1 and the items on both sides of each of the three byte lines, under |hip - fp64| <= 4 |fp32 - fp64| + 2e-6 range (bit for
bit where the op's own test is), and (b) at EVERY item, bit for bit, against the same wrapper on batch slices that stay below 2^31
bytes per operand -- the regime every other test verifies; (c) the device is synchronised after the large launch before anything
is compared.  A batch reduction is checked against the device's FP64 evaluation accumulated over such slices.

A row is skipped only where the device has less free memory than the row's computed peak plus 2 GiB.

Recorded on an MI355X (288 GB): 69 passed, 0 skipped, 26 s for the module; the slowest rows take 6.2 s and 4.2 s (the first launches of
a session), every other one under a second.  Computed peaks run from 10.3 GiB to 30.6 GiB (epe_accum_multi 30.6, add 28.3,
conv2d_k3_multi 25.1, trilinear_ac_soft_argmin_bwd 24.2); the allocator's peak stayed below the computed one in every row, which the
test asserts.  No item-wise row needed a tolerance in (b): every one equals its slices bit for bit, the convolutions on the
single-chain kernels with the same planned form at both batch sizes (tests/test_large_tensors_host.py).  No kernel, wrapper or shim
cast had to be fixed."""
import pytest
import torch

from tests import _large

pytestmark = pytest.mark.gpu

ROWS = _large.rows()


@pytest.fixture(autouse=True)
def _release():
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()        # the large buffers go back to the device before the next row


@pytest.mark.parametrize("row", ROWS, ids=["f%d-%s" % (r.family, r.id) for r in ROWS])
def test_large_tensor(dev, request, row):
    from densematchingbenchmark_amd import ops
    if row.single_chain:
        request.getfixturevalue("single_chain")     # a batch equals its slices bit for bit on the single-chain kernels
    need, (free, _) = row.peak_bytes() + (2 << 30), torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("%s needs %.1f GiB (peak %.1f GiB + 2 GiB), the device has %.1f GiB free" % (row.id, need / 2**30, row.peak_bytes() / 2**30, free / 2**30))
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()        # (what other tests of the session keep alive is not this row's)
    fails = (_large.run_item_row if row.kind == "item" else _large.run_reduce_row)(row, ops, dev)
    print("%s: B %d, computed peak %.1f GiB, allocator peak %.1f GiB" % (row.id, row.B, row.peak_bytes() / 2**30, (torch.cuda.max_memory_allocated() - held) / 2**30))
    assert torch.cuda.max_memory_allocated() - held <= row.peak_bytes(), "the row's computed peak is too low"
    assert not fails, "\n".join(fails)


def test_a_batch_beyond_the_grid_limit_is_refused(dev):
    """Supported or refused, never silently wrong: dmb_cat_fms_bwd_f32 puts B * C on a grid axis (include/dmb_hip.h), so a batch past
    65535 planes -- on tiny items; nothing large is needed to reach the limit -- raises DMB_EUNSUPPORTED before any launch."""
    from densematchingbenchmark_amd import _lib, ops
    dvol = torch.zeros((40000, 4, 2, 2, 8), device=dev)        # cat volume of C = 2 channels: B * C = 80000
    with pytest.raises(_lib.DmbLibraryError, match=str(_lib.DEFINES["DMB_EUNSUPPORTED"])):
        ops.cat_fms_bwd(dvol, [0, 1])
    torch.cuda.synchronize()
