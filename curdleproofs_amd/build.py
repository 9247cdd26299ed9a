"""Builds libcpx.so (HIP kernels + host engine + C-ABI) for gfx950 with hipcc, in-tree.

    python -m curdleproofs_amd.build [--force]

hipcc cross-compiles without a GPU; the resulting curdleproofs_amd/_lib/libcpx.so travels to the
GPU box with the repository snapshot.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "_lib")
LIB = os.path.join(OUT_DIR, "libcpx.so")
ARCH = "gfx950"
SOURCES = ["kernels.hip", "late.hip", "protocol.hip", "round.hip", "tracker.hip", "shuffle.hip", "run.hip", "genmul.hip", "find.hip", "rng.hip", "rng_g1.hip", "engine.cpp", "engine_device.cpp", "whisk.cpp", "capi.cpp"]
# host side: x86-64-v3 + ADX (BMI2 mulx / andn / rorx: the Keccak permutation of the transcripts runs 1.7x faster, the
# 64-bit-limb Fr products use mulx); every host of an MI355X (EPYC 9005) has them
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=" + ARCH, "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-ffp-contract=off",
         "-Xarch_host", "-march=x86-64-v3", "-Xarch_host", "-madx"]

SELFCHECK = os.path.join(OUT_DIR, "quad_selfcheck")
# test-only device program: every field and point operation on raw limbs, one kernel each (tests/test_gpu_field.py).  The
# library does not depend on it: a tree without the tests' source builds libcpx.so alone.
FIELDCHECK = os.path.join(OUT_DIR, "field_check")
FIELDCHECK_SRC = os.path.join(HERE, "..", "tests", "device", "field_check.hip")
# test-only device program: the three transcript implementations at every position of the rate (tests/test_gpu_transcript.py)
TRANSCRIPTCHECK = os.path.join(OUT_DIR, "transcript_check")
TRANSCRIPTCHECK_SRC = os.path.join(HERE, "..", "tests", "device", "transcript_check.hip")
# test-only device program: every function of the scalar-side headers on raw words (tests/test_gpu_scalar.py)
SCALARCHECK = os.path.join(OUT_DIR, "scalar_check")
SCALARCHECK_SRC = os.path.join(HERE, "..", "tests", "device", "scalar_check.hip")
# test-only device program: every function of rng.hpp on raw words (tests/test_gpu_rng.py)
RNGCHECK = os.path.join(OUT_DIR, "rng_check")
RNGCHECK_SRC = os.path.join(HERE, "..", "tests", "device", "rng_check.hip")
# test-only device program: the pieces of G1::rand on raw words (tests/test_gpu_rng_g1.py)
RNGG1CHECK = os.path.join(OUT_DIR, "rng_g1_check")
RNGG1CHECK_SRC = os.path.join(HERE, "..", "tests", "device", "rng_g1_check.hip")
# test-only device program: the MSM wave bodies of msm_body.hpp bucket by bucket and the library's own reducers on crafted sets
# (tests/test_gpu_msm_waves.py); it calls the launchers of kernels.h, so it is linked against the finished libcpx.so beside it
MSMCHECK = os.path.join(OUT_DIR, "msm_check")
MSMCHECK_SRC = os.path.join(HERE, "..", "tests", "device", "msm_check.hip")
DEVICE_FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-I", CSRC]   # the library's device flags


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the MI355X core cannot be built (there is no CPU fallback)")


def _stale():
    check = os.path.exists(FIELDCHECK_SRC)
    tcheck = os.path.exists(TRANSCRIPTCHECK_SRC)
    scheck = os.path.exists(SCALARCHECK_SRC)
    rcheck = os.path.exists(RNGCHECK_SRC)
    mcheck = os.path.exists(MSMCHECK_SRC)
    gcheck = os.path.exists(RNGG1CHECK_SRC)
    outs = ([RNGG1CHECK] if gcheck else []) + [LIB] + ([FIELDCHECK] if check else []) + ([TRANSCRIPTCHECK] if tcheck else []) + ([SCALARCHECK] if scheck else []) + ([RNGCHECK] if rcheck else []) + ([MSMCHECK] if mcheck else [])
    if not all(os.path.exists(o) for o in outs):
        return True
    t = min(os.path.getmtime(o) for o in outs)
    deps = ([RNGG1CHECK_SRC] if gcheck else []) + [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "cpx.h"), __file__] + ([FIELDCHECK_SRC] if check else []) + ([TRANSCRIPTCHECK_SRC] if tcheck else []) + ([SCALARCHECK_SRC] if scheck else []) + ([RNGCHECK_SRC] if rcheck else []) + ([MSMCHECK_SRC] if mcheck else [])
    return any(os.path.getmtime(d) > t for d in deps)


def build_variant(name, defines, verbose=False):
    """Builds an experimental variant libcpx_<name>.so with extra -D flags (A/B runs; select it at load
    time with the CPX_LIB environment variable)."""
    os.makedirs(OUT_DIR, exist_ok=True)
    hipcc = _hipcc()
    out = os.path.join(OUT_DIR, "libcpx_%s.so" % name)
    cmd = [hipcc] + FLAGS + ["-D" + d for d in defines] + ["-shared", "-x", "hip"] + [os.path.join(CSRC, s) for s in SOURCES] + ["-o", out, "-lpthread"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def build(force=False, verbose=False):
    """Builds libcpx.so if any source is newer.  Concurrent callers (a test session and a manual build, several ranks starting at
    once) are serialised by a lock file, objects go to a directory of their own per build and the finished library is moved into
    place atomically: a reader never sees a half-written or mixed-generation libcpx.so."""
    import fcntl
    if not force and not _stale():
        return LIB
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not _stale():      # somebody else built it while we waited
            return LIB
        hipcc = _hipcc()
        work = os.path.join(OUT_DIR, "build.tmp")   # (fixed name: builds are serialised by the lock, and the output stays reproducible)
        shutil.rmtree(work, ignore_errors=True)
        os.makedirs(work)
        try:
            objs = []
            procs = []
            for src in SOURCES:
                obj = os.path.join(work, src + ".o")
                cmd = [hipcc] + FLAGS + (["-x", "hip"] if src.endswith(".cpp") else []) + ["-c", os.path.join(CSRC, src), "-o", obj]
                if verbose:
                    print(" ".join(cmd))
                procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
                objs.append(obj)
            tmp_check = os.path.join(work, "field_check")   # compiles beside the library's sources
            check = os.path.exists(FIELDCHECK_SRC)
            if check:
                procs.append(("field_check.hip", subprocess.Popen(_fieldcheck_cmd(tmp_check), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
            tmp_tcheck = os.path.join(work, "transcript_check")
            tcheck = os.path.exists(TRANSCRIPTCHECK_SRC)
            if tcheck:
                procs.append(("transcript_check.hip", subprocess.Popen(_transcriptcheck_cmd(tmp_tcheck), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
            tmp_scheck = os.path.join(work, "scalar_check")
            scheck = os.path.exists(SCALARCHECK_SRC)
            if scheck:
                procs.append(("scalar_check.hip", subprocess.Popen(_scalarcheck_cmd(tmp_scheck), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
            tmp_rcheck = os.path.join(work, "rng_check")
            rcheck = os.path.exists(RNGCHECK_SRC)
            if rcheck:
                procs.append(("rng_check.hip", subprocess.Popen(_rngcheck_cmd(tmp_rcheck), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
            tmp_gcheck = os.path.join(work, "rng_g1_check")
            gcheck = os.path.exists(RNGG1CHECK_SRC)
            if gcheck:
                procs.append(("rng_g1_check.hip", subprocess.Popen(_rngg1check_cmd(tmp_gcheck), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
            tmp_mobj, tmp_mcheck = os.path.join(work, "msm_check.o"), os.path.join(work, "msm_check")
            mcheck = os.path.exists(MSMCHECK_SRC)
            if mcheck:
                procs.append(("msm_check.hip", subprocess.Popen(_msmcheck_compile_cmd(tmp_mobj), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
            for src, p in procs:
                out, _ = p.communicate()
                if p.returncode != 0:
                    sys.stderr.write(out.decode())
                    raise RuntimeError("hipcc failed on " + src)
                if verbose and out:
                    print(out.decode())
            tmp_lib = os.path.join(work, "libcpx.so")
            subprocess.check_call([hipcc, "-shared", "-fPIC", "--offload-arch=" + ARCH, "-o", tmp_lib] + objs + ["-lpthread"])
            if mcheck:
                subprocess.check_call(_msmcheck_link_cmd(tmp_mobj, work, tmp_mcheck))
            os.replace(tmp_lib, LIB)
            if mcheck:
                os.replace(tmp_mcheck, MSMCHECK)
            if check:
                os.replace(tmp_check, FIELDCHECK)
            if tcheck:
                os.replace(tmp_tcheck, TRANSCRIPTCHECK)
            if scheck:
                os.replace(tmp_scheck, SCALARCHECK)
            if rcheck:
                os.replace(tmp_rcheck, RNGCHECK)
            if gcheck:
                os.replace(tmp_gcheck, RNGG1CHECK)
        finally:
            shutil.rmtree(work, ignore_errors=True)
        build_selfcheck()
    return LIB


def build_selfcheck():
    """The device-side self-check of the quad-cooperative point formulas (g1_28_quad.hpp against the one-lane formulas of
    g1_28.hpp, every special case), an executable that travels with the library; tests/test_gpu_parity.py runs it."""
    os.makedirs(OUT_DIR, exist_ok=True)
    src = os.path.join(HERE, "..", "scripts", "micro", "quad_micro.hip")
    subprocess.check_call([_hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-I", CSRC, src, "-o", SELFCHECK])
    return SELFCHECK


def _fieldcheck_cmd(out):
    return [_hipcc(), "--offload-arch=" + ARCH] + DEVICE_FLAGS + [FIELDCHECK_SRC, "-o", out]


def build_fieldcheck():
    """The device build of tests/device/field_check.hip alone (build() compiles it with the library; the host twin is compiled by
    the tests with g++): cross-compiled here, it travels with the library."""
    if not os.path.exists(FIELDCHECK_SRC):
        raise RuntimeError("tests/device/field_check.hip is missing: the device field check cannot be built")
    os.makedirs(OUT_DIR, exist_ok=True)
    subprocess.check_call(_fieldcheck_cmd(FIELDCHECK + ".tmp"))
    os.replace(FIELDCHECK + ".tmp", FIELDCHECK)
    return FIELDCHECK


def _transcriptcheck_cmd(out):
    return [_hipcc(), "--offload-arch=" + ARCH] + DEVICE_FLAGS + [TRANSCRIPTCHECK_SRC, "-o", out]


def build_transcriptcheck():
    """The device build of tests/device/transcript_check.hip alone (build() compiles it with the library; the host twin is compiled
    by the tests with g++): cross-compiled here, it travels with the library."""
    if not os.path.exists(TRANSCRIPTCHECK_SRC):
        raise RuntimeError("tests/device/transcript_check.hip is missing: the device transcript check cannot be built")
    os.makedirs(OUT_DIR, exist_ok=True)
    subprocess.check_call(_transcriptcheck_cmd(TRANSCRIPTCHECK + ".tmp"))
    os.replace(TRANSCRIPTCHECK + ".tmp", TRANSCRIPTCHECK)
    return TRANSCRIPTCHECK


def _scalarcheck_cmd(out):
    return [_hipcc(), "--offload-arch=" + ARCH] + DEVICE_FLAGS + [SCALARCHECK_SRC, "-o", out]


def build_scalarcheck():
    """The device build of tests/device/scalar_check.hip alone (build() compiles it with the library; the host twin is compiled by
    the tests with g++): cross-compiled here, it travels with the library."""
    if not os.path.exists(SCALARCHECK_SRC):
        raise RuntimeError("tests/device/scalar_check.hip is missing: the device scalar check cannot be built")
    os.makedirs(OUT_DIR, exist_ok=True)
    subprocess.check_call(_scalarcheck_cmd(SCALARCHECK + ".tmp"))
    os.replace(SCALARCHECK + ".tmp", SCALARCHECK)
    return SCALARCHECK


def _rngcheck_cmd(out):
    return [_hipcc(), "--offload-arch=" + ARCH] + DEVICE_FLAGS + [RNGCHECK_SRC, "-o", out]


def build_rngcheck():
    """The device build of tests/device/rng_check.hip alone (build() compiles it with the library; the host twin is compiled by the
    tests with g++): cross-compiled here, it travels with the library."""
    if not os.path.exists(RNGCHECK_SRC):
        raise RuntimeError("tests/device/rng_check.hip is missing: the device rng check cannot be built")
    os.makedirs(OUT_DIR, exist_ok=True)
    subprocess.check_call(_rngcheck_cmd(RNGCHECK + ".tmp"))
    os.replace(RNGCHECK + ".tmp", RNGCHECK)
    return RNGCHECK


def _rngg1check_cmd(out):
    return [_hipcc(), "--offload-arch=" + ARCH] + DEVICE_FLAGS + [RNGG1CHECK_SRC, "-o", out]


def build_rngg1check():
    """The device build of tests/device/rng_g1_check.hip alone (build() compiles it with the library; the host twin is compiled by the
    tests with g++): cross-compiled here, it travels with the library."""
    if not os.path.exists(RNGG1CHECK_SRC):
        raise RuntimeError("tests/device/rng_g1_check.hip is missing: the device G1 rng check cannot be built")
    os.makedirs(OUT_DIR, exist_ok=True)
    subprocess.check_call(_rngg1check_cmd(RNGG1CHECK + ".tmp"))
    os.replace(RNGG1CHECK + ".tmp", RNGG1CHECK)
    return RNGG1CHECK


def _msmcheck_compile_cmd(obj):
    return [_hipcc(), "--offload-arch=" + ARCH] + DEVICE_FLAGS + ["-c", MSMCHECK_SRC, "-o", obj]


def _msmcheck_link_cmd(obj, lib_dir, out):
    # libcpx.so carries no soname: the program records the bare file name and finds the library in its own directory
    return [_hipcc(), "--offload-arch=" + ARCH, obj, "-L", lib_dir, "-lcpx", "-Wl,-rpath,$ORIGIN", "-o", out]


def build_msmcheck():
    """The device build of tests/device/msm_check.hip alone (build() compiles it with the library): cross-compiled here and linked
    against the libcpx.so beside it, it travels with the library."""
    if not os.path.exists(MSMCHECK_SRC):
        raise RuntimeError("tests/device/msm_check.hip is missing: the device MSM check cannot be built")
    if not os.path.exists(LIB):
        raise RuntimeError("libcpx.so is missing: build the library first")
    obj = MSMCHECK + ".tmp.o"
    try:
        subprocess.check_call(_msmcheck_compile_cmd(obj))
        subprocess.check_call(_msmcheck_link_cmd(obj, OUT_DIR, MSMCHECK + ".tmp"))
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    os.replace(MSMCHECK + ".tmp", MSMCHECK)
    return MSMCHECK


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
