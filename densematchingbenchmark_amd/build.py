"""Build recipe for libdmb_hip.so (the C-ABI library declared in include/dmb_hip.h).

Plain ``hipcc --offload-arch=gfx950`` per translation unit, then one ``-shared`` link, all in-tree under
``densematchingbenchmark_amd/lib/`` so that the built library travels with a repository snapshot.
hipcc cross-compiles without a GPU.  Run as ``python -m densematchingbenchmark_amd.build``.
"""
import os
import subprocess
import sys

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_DIR = os.path.join(PKG_DIR, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libdmb_hip.so")
INCLUDE = os.path.join(os.path.dirname(PKG_DIR), "include")

SOURCES = ["core.cpp", "volume.hip", "regression.hip", "conv3d.hip", "conv3d_s1s2.hip", "deconv3d.hip", "conv3d_c1.hip", "confhead.hip", "gwc_mfma.hip", "conv2d.hip", "losses.hip", "conv3d_x6.hip", "wgrad.hip", "norm.hip", "path_bwd.hip", "catconv.hip", "warp_volume.hip", "deconv3d_zy.hip", "conv3d_sk.hip", "spn.hip", "preprocess.hip", "preact_conv.hip", "patch_match.hip", "conv3d_hw.hip", "deeppruner_heads.hip", "refine_head.hip", "deeppruner_final_maps.hip", "deeppruner_loss.hip"]
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
# warp_volume.hip, patch_match.hip and deeppruner_heads.hip restate the reference's FP32 sampler arithmetic (warp_taps.h) operation
# by operation: no fused multiply-adds there (the 5x5 convolution of deeppruner_heads.hip writes its fmaf chain out)
EXTRA_FLAGS = {"warp_volume.hip": ["-ffp-contract=off"], "spn.hip": ["-ffp-contract=off"], "patch_match.hip": ["-ffp-contract=off"],
               "deeppruner_heads.hip": ["-ffp-contract=off"]}
SHARED_HEADERS = ["dmb_common.h", "conv3d_mfma.h", "deconv3d_plan.h", "conv2d_plan.h", "wgrad_plan.h", "upsample_plan.h", "interp.h", "warp_taps.h", "bilinear_hp.h", "loss_terms.h"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def sources_digest(dev=False, defs=""):
    """sha256 over everything a build of the library is made from: every translation unit, the shared headers, the compiler flags
    (and -DDMB_DEV / the build-time experiment's defines).  The linked library carries it (``dmb_build_id()``) and
    ``_lib.load()`` compares it with the digest of the sources next to it: a library that was not built from THESE sources --
    a stale one, or one that travelled to another box with different sources -- is refused instead of silently used."""
    import hashlib
    h = hashlib.sha256()
    for name in SOURCES + SHARED_HEADERS:
        h.update(name.encode())
        h.update(open(os.path.join(CSRC, name), "rb").read())
    h.update(open(os.path.join(INCLUDE, "dmb_hip.h"), "rb").read())
    h.update(repr((ARCH, FLAGS, sorted(EXTRA_FLAGS.items()), bool(dev), defs)).encode())
    return h.hexdigest()


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _unit_digest(src_path, headers, flags):
    """What ONE object file is built from: its translation unit, the shared headers, its compiler flags.  Recorded next to the
    object (<object>.id); an object whose record differs is recompiled whatever the file times say (a checked-out or copied tree
    with mixed times must not link objects of older sources under the new build id)."""
    import hashlib
    h = hashlib.sha256()
    for pth in [src_path] + list(headers):
        h.update(open(pth, "rb").read())
    h.update(repr(flags).encode())
    return h.hexdigest()


def build_library(force=False, verbose=True, dev=False):
    """Compile every HIP source for gfx950 and link libdmb_hip.so.  Returns the library path.

    ``dev=True`` builds the DEVELOPMENT variant instead: the same sources with -DDMB_DEV (kernel-variant switches and diagnostic
    branches for the A/B measurements of scripts/, reached through ``dmb_dev_set_option``) into lib/libdmb_hip_dev.so.  Nothing in
    the package, the tests or bench.py loads it (scripts select it with DMB_LIB=dev); __graft_entry__.build() does not build it."""
    os.makedirs(LIB_DIR, exist_ok=True)
    hipcc = _hipcc()
    lib_path = os.path.join(LIB_DIR, "libdmb_hip_dev.so") if dev else LIB_PATH
    suffix, extra = (".dev.o", ["-DDMB_DEV"]) if dev else (".o", [])
    # build-time experiments (development build only): DMB_BUILD_TAG=st16 DMB_BUILD_DEFS="-DDMB_ZY_ST=16" -> lib/libdmb_hip_dev_st16.so,
    # loaded by scripts with DMB_LIB=dev_st16
    tag = os.environ.get("DMB_BUILD_TAG", "") if dev else ""
    if tag:
        lib_path = os.path.join(LIB_DIR, "libdmb_hip_dev_%s.so" % tag)
        suffix, extra = ".dev_%s.o" % tag, extra + os.environ.get("DMB_BUILD_DEFS", "").split()
    headers = [os.path.join(CSRC, h) for h in SHARED_HEADERS] + [os.path.join(INCLUDE, "dmb_hip.h")]
    # the build id: a generated translation unit that returns the digest of the sources this library is linked from.  If the
    # digest recorded by the previous build differs (whatever the file times say -- a checkout, a copied tree), everything is rebuilt.
    digest = sources_digest(dev, os.environ.get("DMB_BUILD_DEFS", "") if tag else "")
    id_src = os.path.join(LIB_DIR, "build_id%s.gen.cpp" % suffix[:-2])
    id_text = '// generated by build.py\nextern "C" const char* dmb_build_id(void) { return "%s"; }\n' % digest
    digest_changed = not os.path.exists(id_src) or open(id_src).read() != id_text
    if digest_changed:
        with open(id_src, "w") as f:
            f.write(id_text)
    objs, jobs = [], []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        if not os.path.exists(sp):
            raise FileNotFoundError("libdmb_hip.so source listed in build.SOURCES is missing: %s" % sp)
        obj = os.path.join(LIB_DIR, os.path.splitext(src)[0] + suffix)
        objs.append(obj)
        flags = FLAGS + extra + EXTRA_FLAGS.get(src, [])
        unit = _unit_digest(sp, headers, [ARCH] + flags)
        rec = obj + ".id"
        # per-object digest, not file times: an object is reused only if it was built from exactly this unit, headers and flags
        if force or not os.path.exists(obj) or not os.path.exists(rec) or open(rec).read() != unit:
            cmd = [hipcc, "--offload-arch=" + ARCH] + flags + ["-x", "hip", "-c", sp, "-o", obj]
            jobs.append((cmd, rec, unit))
    if jobs:   # the translation units are independent: compile them side by side (bounded by the host's cores)
        from concurrent.futures import ThreadPoolExecutor

        def run(job):
            cmd, rec, unit = job
            if verbose:
                print("[dmb build]", " ".join(cmd), flush=True)
            if os.path.exists(rec):
                os.remove(rec)
            subprocess.check_call(cmd)
            with open(rec, "w") as f:
                f.write(unit)
        with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), os.cpu_count() or 1))) as pool:
            list(pool.map(run, jobs))
    id_obj = os.path.join(LIB_DIR, "build_id" + suffix)
    if force or _stale(id_obj, [id_src]):
        subprocess.check_call([hipcc, "-O1", "-fPIC", "-c", id_src, "-o", id_obj])
    objs.append(id_obj)
    if force or _stale(lib_path, objs):
        # -Bsymbolic: references between the library's own translation units bind inside the library (two builds of it can then
        # be loaded side by side in one process)
        cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-Wl,-Bsymbolic", "-o", lib_path] + objs
        if verbose:
            print("[dmb build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return lib_path


SHIM_SRC = os.path.join(CSRC, "torch_shim.cpp")
SHIM_PATH = os.path.join(LIB_DIR, "_dmb_torch_shim.so")


def shim_digest():
    """What lib/_dmb_torch_shim.so is built from: its one translation unit, the C-ABI header and the torch it is compiled against."""
    import hashlib
    import torch
    h = hashlib.sha256()
    h.update(open(SHIM_SRC, "rb").read())
    h.update(open(os.path.join(INCLUDE, "dmb_hip.h"), "rb").read())
    h.update(torch.__version__.encode())
    return h.hexdigest()


def build_torch_shim(force=False, verbose=True):
    """Compile csrc/torch_shim.cpp -- the thin torch extension over the C ABI (unwrap tensors, current HIP stream, raise on error;
    no device code) -- with the HOST compiler against libtorch / libc10_hip and lib/libdmb_hip.so, in-tree as lib/_dmb_torch_shim.so.
    The library itself must have been built first."""
    import sysconfig
    import torch
    from torch.utils import cpp_extension as ce
    if not os.path.exists(LIB_PATH):
        build_library(verbose=verbose)
    digest = shim_digest()
    stamp = SHIM_PATH + ".id"
    if not force and os.path.exists(SHIM_PATH) and os.path.exists(stamp) and open(stamp).read() == digest:
        return SHIM_PATH
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib")
    cxx = os.environ.get("CXX", "g++")
    cmd = ([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", SHIM_SRC, "-o", SHIM_PATH]
           + ["-I" + p for p in ce.include_paths()]
           + ["-I" + INCLUDE, "-I/opt/rocm/include", "-I" + sysconfig.get_paths()["include"],
              "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1", "-DTORCH_EXTENSION_NAME=_dmb_torch_shim", '-DDMB_SHIM_ID="%s"' % digest,
              "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI), "-Wno-deprecated-declarations",
              "-L" + tlib, "-lc10", "-lc10_hip", "-ltorch_cpu", "-ltorch_hip", "-ltorch", "-ltorch_python",
              "-L" + LIB_DIR, "-ldmb_hip", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + tlib])
    if verbose:
        print("[dmb build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(stamp, "w") as f:
        f.write(digest)
    return SHIM_PATH


if __name__ == "__main__":
    if "--shim" in sys.argv:
        print(build_torch_shim(force="--force" in sys.argv))
        sys.exit(0)

    print(build_library(force="--force" in sys.argv, dev="--dev" in sys.argv))
    if "--dev" not in sys.argv and "--no-shim" not in sys.argv:
        # the release library's torch-extension shim carries a digest of the header: rebuilt here too, so that a library built by hand
        # never travels next to a shim the binding would refuse (and silently fall back to ctypes from)
        print(build_torch_shim(force="--force" in sys.argv, verbose=False))
