"""The table behind tests/test_large_tensors_gpu.py and tests/test_large_tensors_host.py: one row per C-ABI entry point (and
binding) that launches it on an operand of more than 2^31 elements -- past 2 GiB, 4 GiB and 8 GiB of byte offsets at once.

The size comes from the batch count alone: a batch item is one of the small awkward shapes of tests/test_kernels_gpu.py, far
below the per-item limits of include/dmb_hip.h ("Sizes"), and ``B`` is the smallest count that puts the byte offsets 2^31, 2^32
and 2^33 of the large operand strictly inside a batch item.  This module is host-only arithmetic plus the row definitions; the
GPU harness (``run_item_row`` / ``run_reduce_row``) is called by the GPU module only.

A row gives
  entry    the dmb_* name the wrapper launches (the key the host test compares with the header);
  binding  "ctypes" or "shim" for the entry points with a torch-shim path (both run), None for the ctypes-only ones;
  kind     "item" (item b of every output depends on item b of the inputs only) or "reduce" (sums over the batch);
  items    operand -> per-item shape of every batched operand, inputs first, then the outputs in the order ``call`` returns them;
  large    the operand with more than 2^31 elements;
  shared   seed -> the small operands every item shares (weights, affine), on the CPU in FP32;
  call     (ops, batched device tensors, shared device tensors) -> tuple of outputs, through the public wrappers;
  ref      (batched CPU tensors, shared CPU tensors) -> the same outputs by torch / the oracle in the dtype it is handed;
  exact    the outputs the op's existing test compares bit for bit.
"""
import contextlib
import math

import torch
import torch.nn.functional as F

LINES = (1 << 31, 1 << 32, 1 << 33)      # the byte offsets a 32-bit int, a 32-bit unsigned and 2^31 FP32 elements stop at
GRID_LIMIT = 65535                       # the batch count most entry points refuse beyond (grid.y / grid.z, include/dmb_hip.h)
ITEM_LIMIT_BYTES = 1 << 26               # every per-item refusal in csrc/ starts at 2 GiB of some multiple of the item: stay 32x below
PEAK_CAP_BYTES = 40 << 30
NCU = 256                                # compute units the plan queries are asked for (MI355X)

NOT_YET_COVERED = "not yet covered"


def plan_code(lib, plan, B):
    """The host-only plan query of a convolution row at batch count B, every operand 16-byte aligned, single-chain kernels."""
    if plan[0] == "conv3d":
        _, Ci, Co, D, H, W, stride, _ = plan
        return lib.dmb_conv3d_k3_plan(B, Ci, Co, D, H, W, stride, 16, 16, 16, 1, NCU)
    if plan[0] == "deconv3d":
        _, Ci, Co, D, H, W, workspace = plan
        return lib.dmb_deconv3d_k3s2_plan(B, Ci, Co, D, H, W, 2 * W, 16, 16, 16, 16 if workspace else 0, 1, NCU)
    _, Cx, Ci, Co, H, W, k, stride, dil, Ct, _, _ = plan
    return lib.dmb_conv2d_plan(B, Ci, Co, H, W, k, stride, dil, Cx, Ct, 0, 16, 16, 16, 1, NCU)


def _prod(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


class Row:
    def __init__(self, entry, tag, items, inputs, large, shared, call, ref, kind="item", binding=None, exact=(), single_chain=False,
                 dtypes=None, plan=None, scale=None, mean=None, partial=None, finish=None, reduced=(), temps=None):
        self.entry, self.tag, self.items, self.inputs, self.large = entry, tag, dict(items), tuple(inputs), large
        self.shared, self.call, self.ref, self.kind, self.binding = shared, call, ref, kind, binding
        self.exact, self.single_chain, self.plan, self.family = tuple(exact), single_chain, plan, 0
        self.dtypes = dict(dtypes or {})          # operand -> torch dtype where it is not float32
        self.scale = dict(scale or {})            # input -> standard deviation of its values (default 1)
        self.mean = dict(mean or {})              # input -> their mean (default 0)
        self.partial, self.finish = partial, finish     # reduce rows: slice -> additive FP64 sums, sums -> the reduced outputs
        self.reduced = tuple(reduced)             # reduce rows: the names of the outputs ``call`` returns after the batched ones
        self.temps = dict(temps or {})            # name -> per-item shape of what the wrapper allocates besides its outputs
        self.outputs = tuple(n for n in self.items if n not in self.inputs)
        self.also = ()                            # further entry points the row's call launches
        E = _prod(self.items[large])
        self.B = (1 << 31) // E + 2               # the item after the one that holds byte 2^33 is item B - 1

    @property
    def id(self):
        return self.entry[4:] + ("-" + self.tag if self.tag else "") + ("-" + self.binding if self.binding else "")

    def item_bytes(self, name):
        return _prod(self.items[name]) * {torch.int64: 8, torch.float64: 8, torch.uint8: 1}.get(self.dtypes.get(name), 4)

    def checked_items(self):
        """Item 0, item B - 1 and, per byte line of the large operand, the item that holds it and the next: at most 8."""
        ib, s = self.item_bytes(self.large), {0, self.B - 1}
        for line in LINES:
            s.update((line // ib, line // ib + 1))
        return sorted(i for i in s if 0 <= i < self.B)

    def slice_items(self):
        """Batch items per slice of check (b): every operand of a slice stays below 2^31 bytes."""
        per = min(((1 << 31) - 1) // self.item_bytes(n) for n in self.items)
        return per // 4 if self.kind == "reduce" else per      # (a reduction's reference holds FP64 copies of its slice)

    def slices(self):
        per = self.slice_items()
        return [(b0, min(b0 + per, self.B)) for b0 in range(0, self.B, per)]

    def peak_bytes(self):
        """Every batched operand at B items (a residual is the input itself: no buffer of its own), one slice of every output, and as
        much again as the largest slice for the comparison's temporaries."""
        full = sum(self.B * self.item_bytes(n) for n in self.items) + sum(self.B * 4 * _prod(v) for v in self.temps.values())
        per, small = self.slice_items(), 256 << 20      # (weights, workspaces, the items copied for (a))
        if self.kind == "reduce":       # the FP64 copy of a slice of every input and the products summed from it
            return full + small + 4 * per * sum(self.item_bytes(n) for n in self.inputs)
        return (full + small + sum(per * self.item_bytes(n) for n in self.outputs) + sum(per * 4 * _prod(v) for v in self.temps.values())
                + per * max(self.item_bytes(n) for n in self.items))


# ---------------------------------------------------------------------------------------------------- the GPU harness
@contextlib.contextmanager
def binding(which):
    """Run the wrappers through the ctypes binding or through the torch shim (tests/test_kernels_gpu.py switches the same way)."""
    from densematchingbenchmark_amd import _lib
    shim = _lib.shim()
    if which == "shim":
        assert shim is not None, _lib.shim_state()
    try:
        if which == "ctypes":
            _lib._shim = None
        yield
    finally:
        _lib._shim = shim


def _chunks(B, item_bytes):
    per = max(1, ((1 << 31) - 1) // item_bytes)
    return [(b0, min(b0 + per, B)) for b0 in range(0, B, per)]


def _make(row, name, B, dev, gen):
    """A batched input filled on the device, one slice below 2 GiB at a time, so that every item holds different data."""
    dt = row.dtypes.get(name, torch.float32)
    t = torch.empty((B,) + tuple(row.items[name]), dtype=dt, device=dev)
    for b0, b1 in _chunks(B, row.item_bytes(name)):
        if dt == torch.uint8:
            t[b0:b1].random_(0, 256, generator=gen)
        else:
            t[b0:b1].normal_(row.mean.get(name, 0.0), row.scale.get(name, 1.0), generator=gen)
    return t


def _poison(row, B, dev):
    """NaN (int64: -1) where the wrapper's outputs are about to be allocated: the caching allocator hands a block that was just
    freed to the next request of its size, so an element the launch leaves out keeps the sentinel."""
    for name in row.outputs:
        dt = row.dtypes.get(name, torch.float32)
        t = torch.empty((B,) + tuple(row.items[name]), dtype=dt, device=dev)
        for b0, b1 in _chunks(B, row.item_bytes(name)):
            t[b0:b1].fill_(float("nan") if dt.is_floating_point else -1)
        del t


def _has_sentinel(t):
    return bool(torch.isnan(t).any()) if t.dtype.is_floating_point else bool((t < 0).any())


def compare(tag, got, r64, r32, fails):
    """The project's rule (tests/test_unit_grads_gpu.py::_compare without its floor): |hip - fp64| <= 4 |fp32 - fp64| + 2e-6 range."""
    got, r64, r32 = got.detach().cpu().double(), r64.detach().double(), r32.detach().double()
    if got.shape != r64.shape:
        fails.append("%s: shape %s != %s" % (tag, tuple(got.shape), tuple(r64.shape)))
        return
    scale = r64.abs().max().item()
    err = (got - r64).abs().max().item()
    own = (r32 - r64).abs().max().item()
    bound = 4 * own + 2e-6 * scale
    print("%s: error %.3e, bound %.3e (fp32 error %.3e, range %.3e)" % (tag, err, bound, own, scale))
    if not err <= bound:       # (NaN fails too)
        fails.append("%s: error %.3e > bound %.3e (fp32 error %.3e, range %.3e)" % (tag, err, bound, own, scale))


def _to(d, **kw):
    return {k: (v.to(**kw) if isinstance(v, torch.Tensor) and (v.dtype.is_floating_point or "device" in kw) else v) for k, v in d.items()}


def _cast(d, dtype):
    return {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.dtype.is_floating_point else v) for k, v in d.items()}


def _launch_large(row, ops, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    shared = row.shared(seed)
    sdev = _to(shared, device=dev)
    big = {n: _make(row, n, row.B, dev, gen) for n in row.inputs}
    _poison(row, row.B, dev)
    with binding(row.binding):
        outs = row.call(ops, big, sdev)
    torch.cuda.synchronize()        # (c) a wrapped address is a fault, and it surfaces here, before anything is compared
    assert len(outs) == len(row.outputs) + len(row.reduced)
    for n, o in zip(row.outputs, outs):
        assert tuple(o.shape) == (row.B,) + tuple(row.items[n]), (n, tuple(o.shape))
    return big, outs, shared, sdev


def run_item_row(row, ops, dev, seed=20261):
    """Checks (a), (b) and (c) of an item-wise row; -> failure strings."""
    fails = []
    big, outs, shared, sdev = _launch_large(row, ops, dev, seed)
    # (a) plain FP64 / FP32 reference at the items that straddle the three byte lines, and at both ends
    idx = row.checked_items()
    cpu = {n: torch.stack([big[n][i] for i in idx]).cpu() for n in row.inputs}
    r64 = getattr(row, "ref64", row.ref)(_cast(cpu, torch.float64), _cast(shared, torch.float64))
    r32 = row.ref(cpu, shared)
    for n, o, a, b in zip(row.outputs, outs, r64, r32):
        got = torch.stack([o[i] for i in idx]).cpu()
        if n in row.exact:
            if not torch.equal(got, b.to(got.dtype)):
                fails.append("%s %s: items %s differ from the reference, which this op matches bit for bit" % (row.id, n, idx))
        else:
            compare("%s %s items %s" % (row.id, n, idx), got, a, b, fails)
    del cpu, r64, r32
    # (b) every item against the same wrapper on batch slices below 2^31 bytes per operand: bit for bit
    for b0, b1 in row.slices():
        part = {n: big[n][b0:b1] for n in row.inputs}
        _poison(row, b1 - b0, dev)
        with binding(row.binding):
            souts = row.call(ops, part, sdev)
        for n, o, s in zip(row.outputs, outs, souts):
            if _has_sentinel(s):
                fails.append("%s %s: a sentinel survives in the launch on items [%d, %d)" % (row.id, n, b0, b1))
            if not torch.equal(s, o[b0:b1]):        # (a NaN in the large run fails here too: no sentinel survives there either)
                bad = (s != o[b0:b1]).reshape(b1 - b0, -1).any(1).nonzero().view(-1)
                fails.append("%s %s: %d items of [%d, %d) differ from the launch on that slice alone, the first is item %d"
                             % (row.id, n, bad.numel(), b0, b1, b0 + int(bad[0])))
        del souts, part
    torch.cuda.synchronize()
    return fails


def run_reduce_row(row, ops, dev, seed=20262):
    """A batch reduction with elementwise sums: the device's FP64 (and, as the yardstick, FP32) evaluation over slices below 2^31
    bytes, accumulated in FP64, under the rule of (a); -> failure strings."""
    fails = []
    big, outs, shared, sdev = _launch_large(row, ops, dev, seed)
    s64 = s32 = None
    for b0, b1 in row.slices():
        part = {n: big[n][b0:b1] for n in row.inputs}
        p64 = row.partial(_cast(part, torch.float64), _cast(sdev, torch.float64))
        p32 = [p.double() for p in row.partial(part, sdev)]
        s64 = p64 if s64 is None else [a + b for a, b in zip(s64, p64)]
        s32 = p32 if s32 is None else [a + b for a, b in zip(s32, p32)]
        del part
    finish = (lambda sums: row.finish(sums, row.B, sdev)) if row.finish.__code__.co_argcount == 3 else (lambda sums: row.finish(sums, row.B))
    r64, r32 = finish(s64), finish(s32)
    for n, o, a, b in zip(row.reduced, outs[len(row.outputs):], r64, r32):
        compare("%s %s" % (row.id, n), o.reshape(a.shape), a.cpu(), b.cpu(), fails)
    # the elementwise outputs, at every item: the wrapper that applies the large launch's reduced values to a slice, bit for bit
    for b0, b1 in row.slices() if row.outputs else ():
        part = {n: big[n][b0:b1] for n in row.inputs}
        _poison(row, b1 - b0, dev)
        souts = row.elementwise(ops, part, sdev, outs)
        for n, o, e in zip(row.outputs, outs, souts):
            if _has_sentinel(e) or not torch.equal(e, o[b0:b1]):
                fails.append("%s %s: items [%d, %d) differ from the elementwise launch on that slice alone" % (row.id, n, b0, b1))
        del souts, part
    return fails


# ---------------------------------------------------------------------------------------------------- the rows
def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.5 + torch.rand(C, generator=g), torch.rand(C, generator=g) - 0.5


def _bc(v, nd):
    return v.view((1, -1) + (1,) * (nd - 2))


def _conv3d_row(tag, Ci, Co, stride, dhw, relu, residual, binding_, hw=False):
    D, H, W = dhw
    so = (1, 2, 2) if hw else (stride,) * 3
    out = (Co,) + tuple((n - 1) // s + 1 for n, s in zip(dhw, so))

    def shared(seed):
        sc, sh = _affine(Co, seed + 2)
        return {"w": _rand((Co, Ci, 3, 3, 3), seed + 1, 1.0 / math.sqrt(Ci * 27)), "sc": sc, "sh": sh}

    def call(ops, t, s):
        wp = ops.pack_conv3d_weights(s["w"])
        return (ops.conv3d_k3(t["x"], wp, Co, s["sc"], s["sh"], t["x"] if residual else None, so if hw else stride, relu),)

    def ref(t, s):
        y = F.conv3d(t["x"], s["w"], None, stride=so, padding=1) * _bc(s["sc"], 5) + _bc(s["sh"], 5)
        if residual:
            y = y + t["x"]
        return (F.relu(y) if relu else y,)
    return Row("dmb_conv3d_k3_hw_f32" if hw else "dmb_conv3d_k3_f32", tag, {"x": (Ci, D, H, W), "y": out}, ("x",),
               "x" if _prod((Ci, D, H, W)) >= _prod(out) else "y", shared, call, ref, binding=binding_, single_chain=True,
               plan=None if hw else ("conv3d", Ci, Co, D, H, W, stride, bool(residual)))


def _deconv3d_row(tag, Ci, Co, dhw, workspace, binding_, hw=False):
    D, H, W = dhw
    out = (Co, D if hw else 2 * D, 2 * H, 2 * W)

    def shared(seed):
        sc, sh = _affine(Co, seed + 2)
        return {"w": _rand((Ci, Co, 3, 3, 3), seed + 1, 1.0 / math.sqrt(Ci * 27 / 8)), "sc": sc, "sh": sh}

    def call(ops, t, s):
        wp = ops.pack_deconv3d_weights(s["w"])
        if hw:
            return (ops.deconv3d_k3s2(t["x"], wp, Co, s["sc"], s["sh"], None, True, stride=(1, 2, 2)),)
        return (ops.deconv3d_k3s2(t["x"], wp, Co, s["sc"], s["sh"], None, True, workspace=workspace),)

    def ref(t, s):
        y = F.conv_transpose3d(t["x"], s["w"], None, stride=(1, 2, 2) if hw else 2, padding=1, output_padding=(0, 1, 1) if hw else 1)
        return (F.relu(y * _bc(s["sc"], 5) + _bc(s["sh"], 5)),)
    return Row("dmb_deconv3d_k3_hw_f32" if hw else "dmb_deconv3d_k3s2_f32", tag, {"x": (Ci, D, H, W), "y": out}, ("x",), "y", shared, call,
               ref, binding=binding_, single_chain=True, plan=None if hw else ("deconv3d", Ci, Co, D, H, W, workspace is not None))


def _conv3d_c1_row(tag, Ci, dhw, binding_):
    D, H, W = dhw

    def shared(seed):
        return {"w": _rand((1, Ci, 3, 3, 3), seed + 1, 1.0 / math.sqrt(Ci * 27))}

    def call(ops, t, s):
        return (ops.conv3d_k3_c1(t["x"], s["w"], 0.25, None),)

    def ref(t, s):
        return (F.conv3d(t["x"], s["w"], None, padding=1) + 0.25,)
    return Row("dmb_conv3d_k3_c1_f32", tag, {"x": (Ci, D, H, W), "y": (1, D, H, W)}, ("x",), "x", shared, call, ref, binding=binding_,
               single_chain=True)


def _conv2d_row(tag, Ci, Co, k, stride, dil, hw, binding_, window=False):
    H, W = hw
    Cx, Ct = (Ci + 5, Co + 3) if window else (Ci, Co)       # the convolution reads channels [2, 2 + Ci) and writes [3, 3 + Co)
    pad = dil * (k // 2)
    out = (Ct, (H - 1) // stride + 1, (W - 1) // stride + 1)

    def shared(seed):
        sc, sh = _affine(Co, seed + 2)
        return {"w": _rand((Co, Ci, k, k), seed + 1, 1.0 / math.sqrt(Ci * k * k)), "sc": sc, "sh": sh}

    def call(ops, t, s):
        wp = ops.pack_conv2d_weights(s["w"])
        if not window:
            return (ops.conv2d(t["x"], wp, Co, k, stride, dil, s["sc"], s["sh"], None, True),)
        y = torch.full((t["x"].shape[0],) + out, -7.0, device=t["x"].device)
        return (ops.conv2d(t["x"], wp, Co, k, stride, dil, s["sc"], s["sh"], None, True, in_window=(2, Ci), out=y, out_ch_offset=3),)

    def ref(t, s):
        x = t["x"][:, 2:2 + Ci] if window else t["x"]
        y = F.relu(F.conv2d(x, s["w"], None, stride=stride, padding=pad, dilation=dil) * _bc(s["sc"], 4) + _bc(s["sh"], 4))
        if window:
            full = torch.full((y.shape[0],) + out, -7.0, dtype=y.dtype)
            full[:, 3:3 + Co] = y
            y = full
        return (y,)
    return Row("dmb_conv2d_f32", tag, {"x": (Cx, H, W), "y": out}, ("x",), "x" if Cx * H * W >= _prod(out) else "y", shared, call, ref,
               binding=binding_, single_chain=True, plan=("conv2d", Cx, Ci, Co, H, W, k, stride, dil, Ct, 2 if window else 0, 3 if window else 0))


def _gwc_row():
    C, G, H, W, md = 32, 8, 7, 70, 9

    def call(ops, t, s):
        return (ops.gwc_fms(t["L"], t["R"], ops.disp_index_list(md, 0, 1), G),)

    def ref(t, s):
        L, R = t["L"], t["R"]
        out = torch.zeros((L.shape[0], G, md, H, W), dtype=L.dtype)
        for k in range(md):
            out[:, :, k, :, k:] = (L[..., k:] * R[..., :W - k]).view(-1, G, C // G, H, W - k).mean(2)
        return (out,)
    return Row("dmb_gwc_fms_f32", "", {"L": (C, H, W), "R": (C, H, W), "y": (G, md, H, W)}, ("L", "R"), "y", lambda seed: {}, call, ref)


def _conf_head_row():
    D, Cm, H, W = 20, 6, 19, 110

    def shared(seed):
        sc, sh = _affine(Cm, seed + 3)
        return {"w1": _rand((Cm, D, 3, 3), seed + 1, 1.0 / math.sqrt(D * 9)), "w2": _rand((Cm,), seed + 2, 0.5), "sc": sc, "sh": sh}

    def call(ops, t, s):
        return (ops.conf_head(t["cost"], ops.pack_conf_head_weights(s["w1"]), s["sc"], s["sh"], s["w2"]),)

    def ref(t, s):
        h = F.relu(F.conv2d(t["cost"], s["w1"], None, padding=1) * _bc(s["sc"], 4) + _bc(s["sh"], 4))
        return (torch.sigmoid(F.conv2d(h, s["w2"].view(1, Cm, 1, 1))),)
    return Row("dmb_conf_head_f32", "", {"cost": (D, H, W), "conf": (1, H, W)}, ("cost",), "cost", shared, call, ref)


def _volume_row(entry, C, H, W, md, sd, dil):
    """cat_fms / dif_fms / cat_fms_into: pure copies and single subtractions, bit-exact against the oracle."""
    from oracle import dmb_oracle as O
    D = (md + dil - 1) // dil
    into = entry == "dmb_cat_fms_into_f32"
    VC = {"dmb_cat_fms_f32": 2 * C, "dmb_dif_fms_f32": C, "dmb_cat_fms_into_f32": 2 * C + 3}[entry]

    def call(ops, t, s):
        idx = ops.disp_index_list(md, sd, dil)
        if into:
            out = torch.full((t["L"].shape[0], VC, D, H, W), -7.0, device=t["L"].device)
            return (ops.cat_fms_into(t["L"], t["R"], idx, out, 2),)
        return ((ops.dif_fms if entry == "dmb_dif_fms_f32" else ops.cat_fms)(t["L"], t["R"], idx),)

    def ref(t, s):
        if entry == "dmb_dif_fms_f32":
            return (O.dif_fms(t["L"].float(), t["R"].float(), md, sd, dil),)
        y = O.cat_fms(t["L"].float(), t["R"].float(), md, sd, dil)
        if into:
            full = torch.full((y.shape[0], VC, D, H, W), -7.0)
            full[:, 2:2 + 2 * C] = y
            y = full
        return (y,)
    return Row(entry, "", {"L": (C, H, W), "R": (C, H, W), "y": (VC, D, H, W)}, ("L", "R"), "y", lambda seed: {}, call, ref, exact=("y",))


def _correlation_row():
    C, H, W, D = 4, 23, 61, 33

    def call(ops, t, s):
        return (ops.correlation1d(t["L"], t["R"], D, 0.1),)

    def ref(t, s):
        L, R = t["L"], t["R"]
        out = torch.zeros((L.shape[0], D, H, W), dtype=L.dtype)
        for j in range(D):
            d = D - 1 - j
            out[:, j, :, d:] = (L[..., d:] * R[..., :W - d]).sum(1)
        return (F.leaky_relu(out, 0.1),)
    return Row("dmb_correlation1d_f32", "", {"L": (C, H, W), "R": (C, H, W), "y": (D, H, W)}, ("L", "R"), "y", lambda seed: {}, call, ref)


def _soft_argmin_row(entry):
    from oracle import dmb_oracle as O
    D, H, W = 24, 31, 61
    sampled = entry == "dmb_soft_argmin_sampled_f32"

    def call(ops, t, s):
        if sampled:
            return (ops.soft_argmin_sampled(t["cost"], t["sample"], 1.0, True),)
        return (ops.soft_argmin(t["cost"], ops.disp_sample_values(D, 0, 1), 1.0, True),)

    def ref(t, s):
        return (O.soft_argmin(t["cost"], D, disp_sample=t["sample"] if sampled else None),)
    items = {"cost": (D, H, W)}
    if sampled:
        items["sample"] = (D, H, W)
    items["disp"] = (1, H, W)
    return Row(entry, "", items, tuple(n for n in items if n != "disp"), "cost", lambda seed: {}, call, ref,
               scale={"cost": 3.0, "sample": 10.0})


def _local_soft_argmin_row():
    from oracle import dmb_oracle as O
    D, H, W, radius, rd, start, dil = 48, 19, 47, 3, 2, -4, 2

    def call(ops, t, s):
        return ops.local_soft_argmin(t["cost"], radius, rd, start, dil, 1.0, return_index=True)

    def ref(t, s):
        return O.local_soft_argmin(t["cost"], D * dil, radius, start, dil, rd, 1.0)
    return Row("dmb_local_soft_argmin_f32", "", {"cost": (D, H, W), "disp": (1, H, W), "idx": (1, H, W)}, ("cost",), "cost",
               lambda seed: {}, call, ref, exact=("idx",), dtypes={"idx": torch.int64}, scale={"cost": 4.0})


def _trilinear_row(entry, binding_=None):
    # (the form without the volume reads the large operand: its input item carries the size, its output stays small)
    ins, outs = ((8, 64, 65), (9, 65, 67)) if entry == "dmb_trilinear_soft_argmin_f32" else ((5, 12, 16), (19, 45, 61))

    def up(x):
        return F.interpolate(x.unsqueeze(1), list(outs), mode="trilinear", align_corners=True).squeeze(1)

    def regress(y):
        vals = torch.linspace(0, outs[0] - 1, outs[0]).to(y.dtype).view(1, -1, 1, 1)
        return (F.softmax(y, 1) * vals).sum(1, keepdim=True)

    def call(ops, t, s):
        vals = ops.disp_sample_values(outs[0], 0, 1)
        if entry == "dmb_trilinear_ac_f32":
            return (ops.trilinear_ac(t["x"], outs),)
        if entry == "dmb_trilinear_soft_argmin_f32":
            return (ops.trilinear_soft_argmin(t["x"], outs, vals, 1.0),)
        return tuple(ops.trilinear_ac_soft_argmin(t["x"], outs, vals, 1.0))

    def ref(t, s):
        y = up(t["x"])
        return {"dmb_trilinear_ac_f32": (y,), "dmb_trilinear_soft_argmin_f32": (regress(y),)}.get(entry, (y, regress(y)))
    items = {"x": ins}
    if entry != "dmb_trilinear_soft_argmin_f32":
        items["y"] = outs
    if entry != "dmb_trilinear_ac_f32":
        items["disp"] = (1,) + outs[1:]
    return Row(entry, "", items, ("x",), "y" if "y" in items else "x", lambda seed: {}, call, ref, binding=binding_, scale={"x": 3.0})


def _k8s4_row(entry):
    D, H, W = 4, 9, 21
    fused = entry.endswith("soft_argmin_f32")

    def shared(seed):
        return {"w": _rand((8, 8, 8), seed + 1, 0.1)}

    def call(ops, t, s):
        if fused:
            return tuple(ops.deconv3d_k8s4_c1_soft_argmin(t["x"], s["w"], ops.disp_sample_values(4 * D, 0, 1), 1.0))
        return (ops.deconv3d_k8s4_c1(t["x"], s["w"]),)

    def ref(t, s):
        y = F.conv_transpose3d(t["x"].unsqueeze(1), s["w"].view(1, 1, 8, 8, 8), None, stride=4, padding=2).squeeze(1)
        if not fused:
            return (y,)
        vals = torch.linspace(0, 4 * D - 1, 4 * D).to(y.dtype).view(1, -1, 1, 1)
        return (y, (F.softmax(y, 1) * vals).sum(1, keepdim=True))
    items = {"x": (D, H, W), "y": (4 * D, 4 * H, 4 * W)}
    if fused:
        items["disp"] = (1, 4 * H, 4 * W)
    return Row(entry, "", items, ("x",), "y", shared, call, ref, scale={"x": 3.0})


def _stream_row(entry, binding_=None):
    """The streaming ops: a few arithmetic operations per element, one pass."""
    C, H, W = 15, 45, 61
    if entry == "dmb_add_f32":
        return Row(entry, "", {"a": (C, H, W), "b": (C, H, W), "y": (C, H, W)}, ("a", "b"), "a", lambda seed: {},
                   lambda ops, t, s: (ops.add(t["a"], t["b"]),), lambda t, s: (t["a"] + t["b"],))
    if entry == "dmb_copy_window_f32":
        Wd, xs = 48, -3
        return Row(entry, "", {"x": (C, H, W), "y": (C, H, Wd)}, ("x",), "x", lambda seed: {},
                   lambda ops, t, s: (ops.copy_window(t["x"], Wd, xs),),
                   lambda t, s: (F.pad(t["x"], (-xs, max(0, Wd + xs - W)))[..., :Wd],), binding=binding_, exact=("y",))
    if entry == "dmb_zero_columns_f32":
        def ref(t, s):
            y = t["x"].clone()
            y[..., 50:] = 0
            return (y,)
        return Row(entry, "", {"x": (C, H, W), "y": (C, H, W)}, ("x",), "x", lambda seed: {},
                   lambda ops, t, s: (ops.zero_columns_(t["x"].clone(), 50),), ref, exact=("y",))
    if entry == "dmb_bn_act_f32":
        Cb, S = 6, (7, 9, 107)

        def shared(seed):
            sc, sh = _affine(Cb, seed)
            return {"sc": sc, "sh": sh}
        return Row(entry, "", {"c": (Cb,) + S, "y": (Cb,) + S}, ("c",), "c", shared,
                   lambda ops, t, s: (ops.bn_act(t["c"], s["sc"], s["sh"], t["c"], True),),
                   lambda t, s: (F.relu(t["c"] * _bc(s["sc"], 5) + _bc(s["sh"], 5) + t["c"]),))
    if entry == "dmb_avgpool2d_f32":
        k = 8
        return Row(entry, "", {"x": (5, 88, 104), "y": (5, 11, 13)}, ("x",), "x", lambda seed: {},
                   lambda ops, t, s: (ops.avgpool2d(t["x"], k),), lambda t, s: (F.avg_pool2d(t["x"], k, k),))
    if entry == "dmb_bilinear_ac_f32":
        return Row(entry, "", {"x": (5, 23, 27), "y": (5, 89, 93)}, ("x",), "y", lambda seed: {},
                   lambda ops, t, s: (ops.bilinear_ac(t["x"], (89, 93)),),
                   lambda t, s: (F.interpolate(t["x"], (89, 93), mode="bilinear", align_corners=True),))
    if entry == "dmb_bilinear_scale_f32":
        mult = 107.0 / 40
        return Row(entry, "", {"x": (5, 24, 40), "y": (5, 83, 107)}, ("x",), "y", lambda seed: {},
                   lambda ops, t, s: (ops.bilinear_scale(t["x"], (83, 107), mult),),
                   lambda t, s: (F.interpolate(t["x"], (83, 107), mode="bilinear", align_corners=False) * mult,))
    raise KeyError(entry)


def _vjp(f, x, *grads):
    """The plain reference of a backward entry point: autograd through the forward's torch restatement."""
    x = x.detach().clone().requires_grad_(True)
    outs = f(x)
    return torch.autograd.grad(outs if isinstance(outs, tuple) else (outs,), x, grads)[0]


def _volume_bwd_row(entry, C, H, W, md, sd):
    """cat_fms_bwd / dif_fms_bwd: B * C is a grid dimension (at most 65535, include/dmb_hip.h), so the rows take two channels."""
    from oracle import dmb_oracle as O
    dif = entry == "dmb_dif_fms_bwd_f32"
    VC = C if dif else 2 * C

    def call(ops, t, s):
        return (ops.dif_fms_bwd if dif else ops.cat_fms_bwd)(t["dvol"], ops.disp_index_list(md, sd, 1))

    def ref(t, s):
        dv = t["dvol"]
        dL, dR = (torch.zeros((dv.shape[0], C, H, W), dtype=dv.dtype) for _ in range(2))
        for k, d in enumerate(O.disp_index_list(md, sd, 1)):
            if abs(d) >= W:
                continue
            xs, xt = O._valid_x(W, d)
            dL[..., xs] += dv[:, :C, k][..., xs]
            dR[..., xt] += -dv[:, :C, k][..., xs] if dif else dv[:, C:, k][..., xs]
        return dL, dR
    return Row(entry, "", {"dvol": (VC, md, H, W), "dL": (C, H, W), "dR": (C, H, W)}, ("dvol",), "dvol", lambda seed: {}, call, ref)


def _soft_argmin_bwd_row():
    D, H, W = 24, 31, 61

    def regress(c):
        vals = torch.linspace(0, D - 1, D).to(c.dtype).view(1, -1, 1, 1)
        return (F.softmax(c, 1) * vals).sum(1, keepdim=True)

    def call(ops, t, s):
        vals = ops.disp_sample_values(D, 0, 1)
        return (ops.soft_argmin_bwd(t["cost"], ops.soft_argmin(t["cost"], vals, 1.0, True), t["g"], vals, 1.0),)
    return Row("dmb_soft_argmin_bwd_f32", "", {"cost": (D, H, W), "g": (1, H, W), "dcost": (D, H, W)}, ("cost", "g"), "cost",
               lambda seed: {}, call, lambda t, s: (_vjp(regress, t["cost"], t["g"]),), scale={"cost": 3.0}, temps={"disp": (1, H, W)})


def _trilinear_bwd_row(entry):
    ins, outs = (5, 12, 16), (19, 45, 61)
    fused = entry == "dmb_trilinear_ac_soft_argmin_bwd_f32"

    def up(x):
        return F.interpolate(x.unsqueeze(1), list(outs), mode="trilinear", align_corners=True).squeeze(1)

    def both(x):
        y = up(x)
        vals = torch.linspace(0, outs[0] - 1, outs[0]).to(y.dtype).view(1, -1, 1, 1)
        return (F.softmax(y, 1) * vals).sum(1, keepdim=True), y

    def call(ops, t, s):
        if not fused:
            return (ops.trilinear_ac_bwd(t["gy"], ins),)
        vals = ops.disp_sample_values(outs[0], 0, 1)
        disp = ops.trilinear_ac_soft_argmin(t["x"], outs, vals, 1.0)[1]
        return (ops.trilinear_ac_soft_argmin_bwd(t["x"], disp, t["g"], outs, vals, 1.0, grad_cost=t["gy"]),)

    def ref(t, s):
        if not fused:
            return (_vjp(up, torch.zeros((t["gy"].shape[0],) + ins, dtype=t["gy"].dtype), t["gy"]),)
        return (_vjp(both, t["x"], t["g"], t["gy"]),)
    items = {"x": ins, "g": (1,) + outs[1:], "gy": outs, "gx": ins} if fused else {"gy": outs, "gx": ins}
    temps = {"scratch": (ins[0],) + outs[1:]}
    if fused:
        temps.update({"y": outs, "disp": (1,) + outs[1:]})
    return Row(entry, "", items, tuple(n for n in items if n != "gx"), "gy", lambda seed: {}, call, ref, scale={"x": 3.0}, temps=temps)


def _resample_bwd_row(entry):
    if entry == "dmb_avgpool2d_bwd_f32":
        return Row(entry, "", {"gy": (5, 11, 13), "gx": (5, 88, 104)}, ("gy",), "gx", lambda seed: {},
                   lambda ops, t, s: (ops.avgpool2d_bwd(t["gy"], (88, 104), 8),),
                   lambda t, s: (_vjp(lambda x: F.avg_pool2d(x, 8, 8), torch.zeros((t["gy"].shape[0], 5, 88, 104), dtype=t["gy"].dtype), t["gy"]),))
    if entry == "dmb_bilinear_ac_bwd_f32":
        return Row(entry, "", {"gy": (5, 89, 93), "gx": (5, 23, 27)}, ("gy",), "gy", lambda seed: {},
                   lambda ops, t, s: (ops.bilinear_ac_bwd(t["gy"], (23, 27)),),
                   lambda t, s: (_vjp(lambda x: F.interpolate(x, (89, 93), mode="bilinear", align_corners=True),
                                      torch.zeros((t["gy"].shape[0], 5, 23, 27), dtype=t["gy"].dtype), t["gy"]),))
    if entry == "dmb_bilinear_scale_bwd_f32":
        mult = 107.0 / 40
        return Row(entry, "", {"gy": (5, 83, 107), "gx": (5, 24, 40)}, ("gy",), "gy", lambda seed: {},
                   lambda ops, t, s: (ops.bilinear_scale_bwd(t["gy"], (24, 40), mult),),
                   lambda t, s: (_vjp(lambda x: F.interpolate(x, (83, 107), mode="bilinear", align_corners=False) * mult,
                                      torch.zeros((t["gy"].shape[0], 5, 24, 40), dtype=t["gy"].dtype), t["gy"]),))
    if entry == "dmb_deconv3d_k8s4_c1_bwd_f32":     # the data gradient; the weight gradient is a batch reduction
        D, H, W = 4, 9, 21

        def ref(t, s):
            up = lambda x: F.conv_transpose3d(x.unsqueeze(1), s["w"].view(1, 1, 8, 8, 8), None, stride=4, padding=2).squeeze(1)  # noqa: E731
            return (_vjp(up, t["x"], t["dy"]),)
        return Row(entry, "dx", {"x": (D, H, W), "dy": (4 * D, 4 * H, 4 * W), "dx": (D, H, W)}, ("x", "dy"), "dy",
                   lambda seed: {"w": _rand((8, 8, 8), seed + 1, 0.1)},
                   lambda ops, t, s: (ops.deconv3d_k8s4_c1_bwd(t["x"], s["w"], t["dy"], want_dx=True, want_dw=False)[0],), ref)
    raise KeyError(entry)


def _pad_normalize_row(u8):
    Cs, C, sh, sw, win, size = 4, 3, 120, 130, (3, 5, 110, 121), (112, 124)
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)

    def call(ops, t, s):
        return (ops.stereo_pad_normalize(t["src"], size, mean, std, window=win, channels=C),)

    def ref(t, s):
        src = t["src"]
        y0, x0, h, w = win
        crop = src[:, y0:y0 + h, x0:x0 + w, :C].permute(0, 3, 1, 2) if u8 else src[:, :C, y0:y0 + h, x0:x0 + w]
        dt = torch.float32 if u8 and s["dtype"] is None else (s["dtype"] or src.dtype)
        out = torch.zeros((src.shape[0], C) + size, dtype=dt)
        out[:, :, size[0] - h:, :w] = crop.to(dt)
        return ((out - torch.tensor(mean, dtype=dt).view(1, C, 1, 1)) / torch.tensor(std, dtype=dt).view(1, C, 1, 1),)
    if not u8:
        return Row("dmb_stereo_pad_normalize_f32", "", {"src": (Cs, sh, sw), "y": (C,) + size}, ("src",), "src", lambda seed: {"dtype": None},
                   call, ref, scale={"src": 60.0}, mean={"src": 120.0})
    # (the decoder's bytes: the reference in FP64 is asked for through the shared operands, the source has one dtype)
    row = Row("dmb_stereo_pad_normalize_u8", "", {"src": (sh, sw, Cs), "y": (C,) + size}, ("src",), "y", lambda seed: {"dtype": None},
              call, ref, dtypes={"src": torch.uint8})
    row.ref64 = lambda t, s: ref(t, {"dtype": torch.float64})
    return row


def _k5_row():
    Ci, Co, H, W = 16, 5, 45, 61

    def shared(seed):
        sc, sh = _affine(Co, seed + 2)
        return {"w": _rand((Co, Ci, 5, 5), seed + 1, 1.0 / math.sqrt(Ci * 25)), "sc": sc, "sh": sh}
    from densematchingbenchmark_amd import ops_deeppruner
    return Row("dmb_conv2d_k5_small_f32", "", {"x": (Ci, H, W), "y": (Co, H, W)}, ("x",), "x", shared,
               lambda ops, t, s: (ops_deeppruner.conv2d_k5_small(t["x"], s["w"], s["sc"], s["sh"], True),),
               lambda t, s: (F.relu(F.conv2d(t["x"], s["w"], None, padding=2) * _bc(s["sc"], 4) + _bc(s["sh"], 4)),))


def _refine_head_row():
    Ci, H, W = 16, 45, 61
    from densematchingbenchmark_amd import ops_deeppruner

    def ref(t, s):
        y = 2 * F.relu(F.conv2d(t["x"], s["w"], None, padding=1) + t["init"])
        return (F.interpolate(y, scale_factor=2, mode="bilinear", align_corners=False),)
    return Row("dmb_refine_head_up2_f32", "", {"x": (Ci, H, W), "init": (1, H, W), "y": (1, 2 * H, 2 * W)}, ("x", "init"), "x",
               lambda seed: {"w": _rand((1, Ci, 3, 3), seed + 1, 1.0 / math.sqrt(Ci * 9))},
               lambda ops, t, s: (ops_deeppruner.refine_head_up2(t["x"], s["w"], t["init"]),), ref)


def _epe_row(nmaps):
    """dmb_epe_accum_f64 (nmaps 1) / dmb_epe_accum_multi_f64: per image the masked mean error and the outlier percentages
    (oracle/dmb_oracle.py::calc_error on the unpadded maps), summed over the images into float64[6] per estimate."""
    Hp, Wp, H0, W0, lb, ub = 150, 230, 141, 223, 0, 192
    names = ["est%d" % i for i in range(nmaps)]

    def call(ops, t, s):
        acc = torch.zeros((nmaps, 6), dtype=torch.float64, device=t["gt"].device)
        if nmaps == 1:
            ops.epe_accumulate(t["est0"], t["gt"], acc[0], (H0, W0), lb, ub)
        else:
            ops.epe_accumulate_multi([t[n] for n in names], t["gt"], acc, (H0, W0), lb, ub)
        return (acc,)

    def partial(t, s):
        gt = t["gt"][:, :, Hp - H0:, :W0]
        mask = (gt > lb) & (gt < ub)
        n = mask.sum((1, 2, 3)).clamp(min=1).to(gt.dtype)
        rows = []
        for name in names:
            err = (gt - t[name][:, :, Hp - H0:, :W0]).abs()
            per = [torch.full_like(n, 1.0), (err * mask).sum((1, 2, 3)) / n]
            per += [((err > k) & mask).sum((1, 2, 3)).to(gt.dtype) / n * 100 for k in (1, 2, 3, 5)]
            rows.append(torch.stack([p.sum() for p in per]))
        return [torch.stack(rows)]
    items = {n: (1, Hp, Wp) for n in names}
    items["gt"] = (1, Hp, Wp)
    return Row("dmb_epe_accum_f64" if nmaps == 1 else "dmb_epe_accum_multi_f64", "", items, tuple(items), "gt", lambda seed: {}, call, None,
               kind="reduce", partial=partial, finish=lambda sums, B: sums, reduced=("acc",),
               scale={n: 60.0 for n in items}, mean={n: 100.0 for n in items}, temps={"workspace": (nmaps * 2 * 384,)})


def _head_row(chain, binding_):
    """The fused classifier tail (32 -> 32 -> 1 in one launch, csrc/conv3d_s1s2.hip) and, with ``chain``, two of them through
    dmb_conv3d_k3_head_partial_f32 and ONE dmb_conv3d_head_chain_finish_f32.  Tile partial sums added in tile order: reproducible
    and batch-invariant, though not the single chain (the fused form is refused under DMB_CONV_SINGLE_CHAIN)."""
    Ci, D, H, W = 32, 6, 10, 72
    from densematchingbenchmark_amd import ops_head

    def shared(seed):
        out = {}
        for k in range(2 if chain else 1):
            sc, sh = _affine(32, seed + 10 * k + 3)
            out.update({"w%d" % k: _rand((32, Ci, 3, 3, 3), seed + 10 * k + 1, 1.0 / math.sqrt(Ci * 27)), "sc%d" % k: sc, "sh%d" % k: sh,
                        "h%d" % k: _rand((1, 32, 3, 3, 3), seed + 10 * k + 2, 1.0 / math.sqrt(32 * 27))})
        return out

    def call(ops, t, s):
        packs = [(ops.pack_conv3d_weights(s["w%d" % k]), ops_head.pack_conv3d_head_weights(s["h%d" % k])) for k in range(2 if chain else 1)]
        if not chain:
            return (ops_head.conv3d_k3_head(t["x"], packs[0][0], packs[0][1], s["sc0"], s["sh0"], 0.25, None, True),)
        ws = [ops_head.conv3d_k3_head_partial(t["x"], packs[k][0], packs[k][1], s["sc%d" % k], s["sh%d" % k], True) for k in range(2)]
        y = ops_head.conv3d_head_chain_finish(ws, [0.25, -0.5], (t["x"].shape[0], D, H, W))
        return y[0], y[1]

    def level(t, s, k, bias):
        mid = F.relu(F.conv3d(t["x"], s["w%d" % k], None, padding=1) * _bc(s["sc%d" % k], 5) + _bc(s["sh%d" % k], 5))
        return F.conv3d(mid, s["h%d" % k], None, padding=1) + bias

    def ref(t, s):
        y0 = level(t, s, 0, 0.25)
        return (y0, (level(t, s, 1, -0.5) + y0)) if chain else (y0,)
    items = {"x": (Ci, D, H, W), "y0": (1, D, H, W)}
    if chain:
        items["y1"] = (1, D, H, W)
    row = Row("dmb_conv3d_head_chain_finish_f32" if chain else "dmb_conv3d_k3_head_f32", "", items, ("x",), "x", shared, call, ref,
              binding=binding_, temps={"workspace%d" % k: (32768,) for k in range(2 if chain else 1)})
    row.also = ("dmb_conv3d_k3_head_partial_f32",) if chain else ()
    return row


def _x6_row():
    Ci, Co, D, H, W = 32, 32, 6, 10, 48

    def shared(seed):
        sc, sh = _affine(Co, seed + 2)
        return {"w": _rand((Co, Ci, 3, 3, 3), seed + 1, 1.0 / math.sqrt(Ci * 27)), "sc": sc, "sh": sh}

    def call(ops, t, s):
        assert ops.conv3d_x6_applicable(t["x"], Co, 1)
        return (ops.conv3d_k3_x6(t["x"], ops.pack_conv3d_x6_weights(s["w"]), Co, s["sc"], s["sh"], t["x"], True),)

    def ref(t, s):
        return (F.relu(F.conv3d(t["x"], s["w"], None, padding=1) * _bc(s["sc"], 5) + _bc(s["sh"], 5) + t["x"]),)
    return Row("dmb_conv3d_k3_x6_f32", "", {"x": (Ci, D, H, W), "y": (Co, D, H, W)}, ("x",), "x", shared, call, ref)


def _conv2d_multi_row():
    Ci, Co, H, W0, W1 = 32, 32, 20, 72, 24

    def shared(seed):
        return {"w0": _rand((Co, Ci, 3, 3), seed + 1, 1.0 / math.sqrt(Ci * 9)), "w1": _rand((Co, Ci, 3, 3), seed + 2, 1.0 / math.sqrt(Ci * 9))}

    def call(ops, t, s):
        B, dev = t["x0"].shape[0], t["x0"].device
        y0 = torch.full((B, Co + 3, H, W0), -7.0, device=dev)
        y1 = torch.empty((B, Co, H, W1), device=dev)
        ops.conv2d_k3_multi([(t["x0"], ops.pack_conv2d_weights(s["w0"]), y0, 3), (t["x1"], ops.pack_conv2d_weights(s["w1"]), y1, 0)], Co)
        return y0, y1

    def ref(t, s):
        y0 = F.conv2d(t["x0"], s["w0"], None, padding=1)
        full = torch.full((y0.shape[0], Co + 3, H, W0), -7.0, dtype=y0.dtype)
        full[:, 3:] = y0
        return full, F.conv2d(t["x1"], s["w1"], None, padding=1)
    return Row("dmb_conv2d_k3_multi_f32", "", {"x0": (Ci, H, W0), "x1": (Ci, H, W1), "y0": (Co + 3, H, W0), "y1": (Co, H, W1)},
               ("x0", "x1"), "y0", shared, call, ref)


def _anynet_samples_row():
    h, w, H, W, D, scale = 12, 25, 45, 97, 9, 2.0

    def call(ops, t, s):
        return ops.anynet_stage_samples(t["low"], (H, W), scale, s["lin"])

    def ref(t, s):
        up = F.interpolate(t["low"] * scale, (H, W), mode="bilinear", align_corners=False)
        return up, s["lin"].view(1, D, 1, 1) + up
    return Row("dmb_anynet_stage_samples_f32", "", {"low": (1, h, w), "up": (1, H, W), "samples": (D, H, W)}, ("low",), "samples",
               lambda seed: {"lin": torch.linspace(-3.0, 3.0, D)}, call, ref, scale={"low": 10.0})


def _uniform_samples_row():
    """The range head of stage "post" and the uniform sampler: bit for bit the reference's FP32 arithmetic
    (tests/test_deeppruner_sampler_gpu.py compares with torch.equal)."""
    from tests import _deeppruner_ref as R
    H, W, N, max_disp = 45, 97, 9, 48.0

    def ref(t, s):
        lo, hi = R.range_head_post(t["lo"].float(), t["hi"].float(), N, max_disp)
        return (R.uniform_samples(lo, hi, N),)
    return Row("dmb_deeppruner_uniform_samples_f32", "", {"lo": (1, H, W), "hi": (1, H, W), "y": (N, H, W)}, ("lo", "hi"), "y",
               lambda seed: {}, lambda ops, t, s: (ops.deeppruner_uniform_samples(t["lo"], t["hi"], N, max_disp),), ref, exact=("y",),
               scale={"lo": 12.0, "hi": 12.0}, mean={"lo": 12.0, "hi": 30.0})


def _bn_train_fwd_row(binding_):
    """Batch statistics + normalisation in two launches.  The statistics are the batch reduction; y is elementwise GIVEN them, so
    every item of it is compared, bit for bit, with dmb_bn_act_f32 on slices fed the scale / shift of the large launch (the two
    kernels apply the same fmaf / fmaxf sequence, csrc/norm.hip)."""
    C, S = 6, (7, 9, 107)
    n = _prod(S)

    def shared(seed):
        g, b = _affine(C, seed + 1)
        return {"gamma": g, "beta": b}

    def call(ops, t, s):
        return ops.bn_train_fwd(t["c"], s["gamma"], s["beta"], None, None, None, 0.1, 1e-5, t["c"], True)

    def partial(t, s):
        c = t["c"]
        return [c.sum((0, 2, 3, 4)), (c * c).sum((0, 2, 3, 4))]

    def finish(sums, B, s):
        mean = sums[0] / (B * n)
        invstd = (sums[1] / (B * n) - mean * mean + 1e-5).rsqrt()
        scale = s["gamma"].double() * invstd
        return [mean, invstd, scale, s["beta"].double() - mean * scale]

    def elementwise(ops, t, s, outs):
        return (ops.bn_act(t["c"], outs[3], outs[4], t["c"], True),)
    row = Row("dmb_bn_train_fwd_f32", "", {"c": (C,) + S, "y": (C,) + S}, ("c",), "c", shared, call, None, kind="reduce", binding=binding_,
              partial=partial, finish=finish, reduced=("mean", "invstd", "scale", "shift"), mean={"c": 0.5})
    row.elementwise = elementwise
    return row


def _channel_dot_row():
    C, S = 6, (7, 9, 107)

    def partial(t, s):
        return [(t["a"] * t["g"]).sum((0, 2, 3, 4))]
    return Row("dmb_channel_dot_f32", "", {"a": (C,) + S, "g": (1,) + S}, ("a", "g"), "a", lambda seed: {},
               lambda ops, t, s: (ops.channel_dot(t["a"], t["g"]),), None, kind="reduce", partial=partial, finish=lambda sums, B: sums, reduced=("out",),
               mean={"a": 0.5, "g": 0.5})    # (sums of zero-mean products would leave the rule's 2e-6 * range without a range)


def _bn_stats_row():
    C, S = 6, (7, 9, 107)
    n = _prod(S)

    def partial(t, s):
        c = t["c"]
        return [c.sum((0, 2, 3, 4)), (c * c).sum((0, 2, 3, 4))]

    def finish(sums, B):
        mean = sums[0] / (B * n)
        var = sums[1] / (B * n) - mean * mean
        return [mean, (var + 1e-5).rsqrt()]
    return Row("dmb_bn_train_stats_f32", "", {"c": (C,) + S}, ("c",), "c", lambda seed: {},
               lambda ops, t, s: tuple(ops.bn_train_stats(t["c"])[:2]), None, kind="reduce", partial=partial, finish=finish, reduced=("mean", "invstd"),
               mean={"c": 0.5})              # (a channel mean of ~0 would leave the rule's 2e-6 * range without a range)


# The issue's four families: 1 = the MFMA / LDS-DMA kernels, 2 = the volume builders and regression ends, 3 = the streaming ops,
# 4 = the batch reductions, backward and loss entry points.
def rows():
    families = {1: [
        _conv3d_row("s1_32to32_res_relu", 32, 32, 1, (6, 10, 70), True, True, "shim"),
        _conv3d_row("s1_32to32_res_relu", 32, 32, 1, (6, 10, 70), True, True, "ctypes"),
        _conv3d_row("s1_32to32_vec", 32, 32, 1, (6, 10, 72), True, True, "shim"),
        _conv3d_row("s1_64to64", 64, 64, 1, (5, 9, 48), False, False, "shim"),
        _conv3d_row("s2_32to64", 32, 64, 2, (6, 11, 96), True, False, "shim"),
        _conv3d_row("s1_20to32", 20, 32, 1, (6, 11, 37), True, False, "shim"),
        _deconv3d_row("queue_64to32", 64, 32, (3, 5, 24), "auto", "shim"),
        _deconv3d_row("queue_64to32", 64, 32, (3, 5, 24), "auto", "ctypes"),
        _deconv3d_row("parity_64to64", 64, 64, (3, 5, 35), None, "shim"),
        _conv3d_c1_row("32", 32, (6, 9, 70), "shim"),
        _conv3d_c1_row("32", 32, (6, 9, 70), "ctypes"),
        _conv3d_row("s122_32to32", 32, 32, 1, (4, 9, 35), True, False, None, hw=True),
        _deconv3d_row("s122_32to16", 32, 16, (4, 9, 21), "auto", None, hw=True),
        _conv2d_row("k3_32to32", 32, 32, 3, 1, 1, (20, 70), "shim"),
        _conv2d_row("k3_32to32", 32, 32, 3, 1, 1, (20, 70), "ctypes"),
        _conv2d_row("k1_64to32", 64, 32, 1, 1, 1, (11, 61), "shim"),
        _conv2d_row("k3_dil4_32to32", 32, 32, 3, 1, 4, (21, 70), "shim"),
        _conv2d_row("k3_windows", 32, 64, 3, 1, 1, (9, 100), "shim", window=True),
        _gwc_row(),
        _conf_head_row(),
        _k5_row(),
        _refine_head_row(),
        _head_row(False, "shim"),
        _head_row(False, "ctypes"),
        _head_row(True, "shim"),
        _head_row(True, "ctypes"),
        _x6_row(),
        _conv2d_multi_row(),
    ], 2: [
        _volume_row("dmb_cat_fms_f32", 5, 7, 61, 12, -3, 1),
        _volume_row("dmb_dif_fms_f32", 8, 15, 61, 12, 0, 2),
        _volume_row("dmb_cat_fms_into_f32", 5, 7, 61, 12, 0, 1),
        _correlation_row(),
        _soft_argmin_row("dmb_soft_argmin_f32"),
        _soft_argmin_row("dmb_soft_argmin_sampled_f32"),
        _local_soft_argmin_row(),
        _trilinear_row("dmb_trilinear_ac_f32"),
        _trilinear_row("dmb_trilinear_ac_soft_argmin_f32", "shim"),
        _trilinear_row("dmb_trilinear_ac_soft_argmin_f32", "ctypes"),
        _trilinear_row("dmb_trilinear_soft_argmin_f32"),
        _k8s4_row("dmb_deconv3d_k8s4_c1_f32"),
        _k8s4_row("dmb_deconv3d_k8s4_c1_soft_argmin_f32"),
        _uniform_samples_row(),
    ], 3: [
        _stream_row("dmb_bn_act_f32"),
        _stream_row("dmb_add_f32"),
        _stream_row("dmb_copy_window_f32", "shim"),
        _stream_row("dmb_copy_window_f32", "ctypes"),
        _stream_row("dmb_zero_columns_f32"),
        _stream_row("dmb_avgpool2d_f32"),
        _stream_row("dmb_bilinear_ac_f32"),
        _stream_row("dmb_bilinear_scale_f32"),
        _anynet_samples_row(),
        _pad_normalize_row(False),
        _pad_normalize_row(True),
    ], 4: [
        _volume_bwd_row("dmb_cat_fms_bwd_f32", 2, 31, 61, 12, -3),
        _volume_bwd_row("dmb_dif_fms_bwd_f32", 2, 45, 61, 12, 0),
        _soft_argmin_bwd_row(),
        _trilinear_bwd_row("dmb_trilinear_ac_bwd_f32"),
        _trilinear_bwd_row("dmb_trilinear_ac_soft_argmin_bwd_f32"),
        _resample_bwd_row("dmb_avgpool2d_bwd_f32"),
        _resample_bwd_row("dmb_bilinear_ac_bwd_f32"),
        _resample_bwd_row("dmb_bilinear_scale_bwd_f32"),
        _resample_bwd_row("dmb_deconv3d_k8s4_c1_bwd_f32"),
        _bn_stats_row(),
        _bn_train_fwd_row("shim"),
        _bn_train_fwd_row("ctypes"),
        _channel_dot_row(),
        _epe_row(1),
        _epe_row(2),
    ]}
    out = []
    for fam, rs in families.items():
        for r in rs:
            r.family = fam
            out.append(r)
    return out
