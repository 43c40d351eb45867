"""The binding on the CPU: the ctypes table parsed from include/dmb_hip.h (pinned for one entry point of each type class, refusals
of what it cannot map), ``_lib.launch`` against a fake library (no device: what it marshals, what it refuses before the call) and
the header's defines behind the package's public constants."""
import ctypes

import pytest
import torch

from densematchingbenchmark_amd import _lib, ops, ops_deeppruner

I, LL, F, D, P, S = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_char_p
HI, HF = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)

PINNED = {
    "dmb_cat_fms_f32": (I, [(P, "L"), (P, "R"), (P, "out"), (I, "B"), (I, "C"), (I, "H"), (I, "W"), (I, "D"), (HI, "disp_idx_host"),
                            (P, "stream")]),
    "dmb_copy_window_f32": (I, [(P, "src"), (P, "dst"), (LL, "rows"), (I, "W"), (I, "Wd"), (I, "xs"), (P, "stream")]),
    "dmb_conv3d_packed_floats": (LL, [(I, "Co"), (I, "Ci")]),
    "dmb_last_error": (S, []),
    "dmb_stereo_pad_normalize_u8": (I, [(P, "src_hwc"), (P, "dst")] + [(I, n) for n in ("B", "C", "Cs", "sh", "sw", "y0", "x0", "h", "w",
                                                                                        "th", "tw")]
                                    + [(HF, "mean_host"), (HF, "std_host"), (P, "stream")]),
    "dmb_deeppruner_loss_fwd_f32": (I, [(P, "d0"), (P, "d1"), (P, "d2"), (HI, "h_host"), (HI, "w_host"), (P, "min_disp"), (P, "max_disp"),
                                        (P, "gt"), (P, "workspace"), (P, "loss_out"), (P, "stats")]
                                    + [(I, n) for n in ("K", "B", "h", "w", "H", "W")]
                                    + [(F, n) for n in ("l1_lower", "l1_upper", "q_lower", "q_upper")] + [(D, "theta"), (P, "stream")]),
    "dmb_epe_accum_multi_f64": (I, [(I, "nmaps"), (P, "est"), (P, "gt"), (P, "acc"), (P, "workspace")]
                                + [(I, n) for n in ("B", "Hp", "Wp", "H0", "W0")] + [(F, "lb"), (F, "ub"), (P, "stream")]),
}


@pytest.mark.parametrize("name", list(PINNED))
def test_parsed_signature(name):
    res, params = PINNED[name]
    assert _lib.PROTOTYPES[name] == (res, params)
    assert _lib.SIGNATURES[name] == (res, [t for t, _ in params])


def test_the_parser_misses_nothing_and_skips_nothing():
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES) == set(_lib.PROTOTYPES)
    protos, defines = _lib.parse_header("#define DMB_A 0x10 /* c */\n#define DMB_B 7\n#define DMB_HIP_H\n"
                                        "/* int dmb_commented(int a); */\nconst char* dmb_s(void);\n"
                                        "long long dmb_q(const float* const* a, double* b_host_not, const float* v_host, long long n);\n")
    assert defines == {"DMB_A": 16, "DMB_B": 7}
    assert protos == {"dmb_s": (S, []), "dmb_q": (LL, [(P, "a"), (P, "b_host_not"), (HF, "v_host"), (LL, "n")])}
    for bad in ("int dmb_x(size_t n, void* stream);", "int dmb_x(struct job* jobs, void* stream);", "unsigned dmb_x(int n);",
                "int dmb_x(const double* v_host, void* stream);", "int dmb_x(const int* const* v_host, void* stream);",
                "int dmb_x(int, void* stream);", "int dmb_x(int (*cb)(int), void* stream);"):
        with pytest.raises(_lib.DmbLibraryError, match="dmb_x"):
            _lib.parse_header("int dmb_ok(int a);\n" + bad + "\n")


class FakeLibrary:
    """Records what an entry point receives; ``code``: what it returns."""

    def __init__(self, code=0):
        self.code, self.calls = code, []

    def __getattr__(self, name):
        if name == "dmb_last_error":
            return lambda: b"the fake's last error"

        def entry(*args):
            self.calls.append((name, args))
            return self.code
        return entry


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLibrary()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "stream_ptr", lambda device=None: ("stream of", device))
    return lib


def test_launch_marshals_by_the_header(fake):
    win, mean = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)
    # dmb_stereo_pad_normalize_f32(src, dst, 11 ints, mean_host, std_host): pointers pass through, sequences become host arrays
    _lib.launch("dmb_stereo_pad_normalize_f32", win, mean, True, 3.0, 3, 4, 5, 0, 0, 4, 5, 4, 8, (1, 2.5, 3), _lib.opt(None), device="dev")
    (name, args), = fake.calls
    assert name == "dmb_stereo_pad_normalize_f32" and len(args) == 16
    assert args[0] is win and args[1] is mean                                  # ctypes pointers pass through untouched
    assert args[2:13] == (1, 3, 3, 4, 5, 0, 0, 4, 5, 4, 8) and all(type(a) is int for a in args[2:13])
    assert isinstance(args[13], ctypes.c_float * 3) and list(args[13]) == [1.0, 2.5, 3.0]
    assert args[14] is None                                                    # the stated-absent operand arrives as NULL
    assert args[15] == ("stream of", "dev")
    # a host int array, an absent device pointer, a pointer array, float / double scalars
    arr = (ctypes.c_void_p * 2)(1, 2)
    _lib.launch("dmb_deeppruner_loss_fwd_f32", win, _lib.opt(None), _lib.NULL, [4, 5], (6, 7), win, win, win, win, win, win, 1, 2, 3, 4,
                5, 6, 0, 192, 0, 192, 0.05, device="dev")
    args = fake.calls[-1][1]
    assert args[1] is None and args[2] is None and isinstance(args[3], ctypes.c_int * 2) and list(args[4]) == [6, 7]
    assert args[17:22] == (0.0, 192.0, 0.0, 192.0, 0.05) and all(type(a) is float for a in args[17:22])
    _lib.launch("dmb_epe_accum_multi_f64", 2, arr, win, win, win, 1, 8, 8, 8, 8, 0, 192, device="dev")
    assert fake.calls[-1][1][1] is arr
    ready = _lib.host_ints([1, 2])
    _lib.launch("dmb_cat_fms_f32", win, win, win, 1, 1, 1, 1, 2, ready, device="dev")
    assert fake.calls[-1][1][8] is ready


def test_launch_refuses_before_the_call(fake):
    win = ctypes.c_void_p(0x1000)
    with pytest.raises(_lib.DmbLibraryError, match=r"dmb_cat_fms_f32: R lives on cpu.*no CPU fallback"):
        _lib.launch("dmb_cat_fms_f32", win, torch.zeros(4), win, 1, 1, 1, 1, 1, [0], device="dev")
    with pytest.raises(_lib.DmbLibraryError, match="dmb_cat_fms_f32: out is None"):
        _lib.launch("dmb_cat_fms_f32", win, win, None, 1, 1, 1, 1, 1, [0], device="dev")
    with pytest.raises(_lib.DmbLibraryError, match="dmb_cat_fms_f32: disp_idx_host is None"):
        _lib.launch("dmb_cat_fms_f32", win, win, win, 1, 1, 1, 1, 1, None, device="dev")
    with pytest.raises(_lib.DmbLibraryError, match="dmb_cat_fms_f32: L must be a torch.Tensor"):
        _lib.launch("dmb_cat_fms_f32", 0x1000, win, win, 1, 1, 1, 1, 1, [0], device="dev")
    for args in ((win, win, win, 1, 1, 1, 1, 1), (win, win, win, 1, 1, 1, 1, 1, [0], 0)):
        with pytest.raises(_lib.DmbLibraryError, match="dmb_cat_fms_f32 takes 9 arguments before the stream, got %d" % len(args)):
            _lib.launch("dmb_cat_fms_f32", *args, device="dev")
    with pytest.raises(_lib.DmbLibraryError, match="no tensor among the operands"):
        _lib.launch("dmb_cat_fms_f32", win, win, win, 1, 1, 1, 1, 1, [0])
    for query in ("dmb_conv3d_packed_floats", "dmb_abi_version", "dmb_conv3d_k3_plan", "dmb_no_such_entry"):
        with pytest.raises(_lib.DmbLibraryError, match="takes a stream"):
            _lib.launch(query, 32, 32, device="dev")
    assert fake.calls == []


def test_launch_raises_on_a_nonzero_code(fake):
    fake.code = 100001
    with pytest.raises(_lib.DmbLibraryError, match=r"dmb_add_f32 failed with code 100001 \(the fake's last error\)"):
        _lib.launch("dmb_add_f32", ctypes.c_void_p(1), ctypes.c_void_p(2), ctypes.c_void_p(3), 4, device="dev")
    assert len(fake.calls) == 1


def test_wrappers_on_cpu_tensors_name_the_parameter_and_launch_nothing(fake):
    t = torch.zeros((1, 2, 4, 8))
    with pytest.raises(_lib.DmbLibraryError, match="dmb_cat_fms_f32: L lives on cpu"):
        ops.cat_fms(t, t, [0, 1])
    with pytest.raises(_lib.DmbLibraryError, match="dmb_add_f32: a lives on cpu"):
        ops.add(t, t)
    assert fake.calls == []


def test_every_launching_entry_point_has_a_plan():
    with_stream = {n for n, (_, params) in _lib.PROTOTYPES.items() if params and params[-1][1] == "stream"}
    assert set(_lib._LAUNCH) == with_stream and "dmb_add_f32" in with_stream and "dmb_conv3d_packed_floats" not in with_stream
    assert all(len(_lib._LAUNCH[n]) == len(_lib.SIGNATURES[n][1]) - 1 for n in with_stream)
    assert not any(p == "stream" for n in _lib.PROTOTYPES for _, p in _lib.PROTOTYPES[n][1][:-1])


def test_public_constants_are_the_headers_defines():
    d = _lib.DEFINES
    assert _lib.ABI_VERSION == d["DMB_ABI_VERSION"]
    assert _lib.DECONV3D_WORKSPACE_BYTES == d["DMB_DECONV3D_WORKSPACE_BYTES"] == 2048
    assert _lib.CONV_SINGLE_CHAIN == d["DMB_CONV_SINGLE_CHAIN"] == 0x100
    assert _lib.CONV3D_HEAD_PACKED_FLOATS == d["DMB_CONV3D_HEAD_PACKED_FLOATS"] == 1024
    assert _lib.DEEPPRUNER_LOSS_WORKSPACE_DOUBLES == d["DMB_DEEPPRUNER_LOSS_WORKSPACE_DOUBLES"] == 9216
    assert ops.MAX_DISP_SAMPLES == d["DMB_MAX_DISP_SAMPLES"] == 256
    assert ops.PATCH_MATCH_MAX_SAMPLES == d["DMB_PATCH_MATCH_MAX_SAMPLES"] == 85
    assert (ops.PREACT_POOL, ops.PREACT_RELU_IN, ops.PREACT_RELU_OUT, ops.PREACT_GATE) == (1, 2, 4, 8) == tuple(
        d["DMB_PREACT_" + n] for n in ("POOL", "RELU_IN", "RELU_OUT", "GATE"))
    assert (ops.PREACT_MAX_CI, ops.PREACT_MAX_CO) == (d["DMB_PREACT_MAX_CI"], d["DMB_PREACT_MAX_CO"]) == (64, 32)
    assert ops.EPE_WORKSPACE_DOUBLES_PER_IMAGE == d["DMB_EPE_WORKSPACE_DOUBLES"] == 384
    assert ops_deeppruner.K5_MAX_C == d["DMB_CONV2D_K5_MAX_C"] == 16
    assert ops_deeppruner.MAX_FEATURE_PLANES == d["DMB_PATCH_MATCH_MAX_SAMPLES"]
    assert ops_deeppruner.REFINE_HEAD_MAX_C == d["DMB_REFINE_HEAD_MAX_C"] == 16
    assert (d["DMB_OK"], d["DMB_EINVAL"], d["DMB_EUNSUPPORTED"]) == (0, 100001, 100002)
