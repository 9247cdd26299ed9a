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
SOURCES = ["kernels.hip", "late.hip", "protocol.hip", "round.hip", "loop.hip", "subarg.hip", "subarg_prove.hip", "gprod.hip", "same_perm.hip", "tracker.hip", "shuffle.hip", "run.hip", "genmul.hip", "find.hip", "rng.hip", "rng_g1.hip", "engine.cpp", "engine_subarg.cpp", "engine_device.cpp", "whisk.cpp", "capi.cpp"]
# host side: x86-64-v3 + ADX (BMI2 mulx / andn / rorx: the Keccak permutation of the transcripts runs 1.7x faster, the
# 64-bit-limb Fr products use mulx); every host of an MI355X (EPYC 9005) has them
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=" + ARCH, "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-ffp-contract=off",
         "-Xarch_host", "-march=x86-64-v3", "-Xarch_host", "-madx"]

SELFCHECK = os.path.join(OUT_DIR, "quad_selfcheck")
# test-only device programs (tests/device/<name>.hip, one per tests/test_gpu_*.py that names it): every function of a header on raw
# words.  The library does not depend on them: a tree without the tests' sources builds libcpx.so alone.  A `standalone` program is one
# hipcc line; the `linked` one calls the launchers of kernels.h, so it is linked against the finished libcpx.so beside it.
CHECKS = {name: (os.path.join(HERE, "..", "tests", "device", name + ".hip"), kind) for name, kind in (
    ("field_check", "standalone"), ("transcript_check", "standalone"), ("scalar_check", "standalone"), ("rng_check", "standalone"),
    ("rng_g1_check", "standalone"), ("msm_check", "linked"), ("quad_check", "standalone"))}
DEVICE_FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-I", CSRC]   # the library's device flags


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the MI355X core cannot be built (there is no CPU fallback)")


def check_path(name):
    return os.path.join(OUT_DIR, name)


def check_source(name):
    return CHECKS[name][0]


# the programs' paths under the names they had before check_path() / check_source(): the tests of the previous commit import them,
# and those tests are run against this build as they stand (the six programs of that commit; later ones have no such name)
FIELDCHECK, TRANSCRIPTCHECK, SCALARCHECK, RNGCHECK, RNGG1CHECK, MSMCHECK = (check_path(name) for name in list(CHECKS)[:6])
MSMCHECK_SRC = check_source("msm_check")


def _check_cmds(name, out, lib_dir):
    """the command lines that make the check program `name` at `out`: the compile (for the linked kind: to out + ".o") and, for the
    linked kind, the link against the libcpx.so of `lib_dir`"""
    compile_ = [_hipcc(), "--offload-arch=" + ARCH] + DEVICE_FLAGS
    if CHECKS[name][1] == "standalone":
        return compile_ + [check_source(name), "-o", out], None
    # libcpx.so carries no soname: the program records the bare file name and finds the library in its own directory
    return compile_ + ["-c", check_source(name), "-o", out + ".o"], [_hipcc(), "--offload-arch=" + ARCH, out + ".o", "-L", lib_dir, "-lcpx", "-Wl,-rpath,$ORIGIN", "-o", out]


def _present_checks():
    return [name for name in CHECKS if os.path.exists(check_source(name))]


def _stale():
    checks = _present_checks()
    outs = [LIB] + [check_path(c) for c in checks]
    if not all(os.path.exists(o) for o in outs):
        return True
    t = min(os.path.getmtime(o) for o in outs)
    # what the check programs share, counted where it exists: a check program whose source is complete in itself builds without it
    harness = os.path.join(HERE, "..", "tests", "device", "check_harness.hpp")
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "cpx.h"), __file__] + [check_source(c) for c in checks]
    return any(os.path.getmtime(d) > t for d in deps + ([harness] if os.path.exists(harness) else []))


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
            checks = {name: _check_cmds(name, os.path.join(work, name), work) for name in _present_checks()}   # compile beside the library's sources
            for name, (compile_, _) in checks.items():
                procs.append((name + ".hip", subprocess.Popen(compile_, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
            for src, p in procs:
                out, _ = p.communicate()
                if p.returncode != 0:
                    sys.stderr.write(out.decode())
                    raise RuntimeError("hipcc failed on " + src)
                if verbose and out:
                    print(out.decode())
            tmp_lib = os.path.join(work, "libcpx.so")
            subprocess.check_call([hipcc, "-shared", "-fPIC", "--offload-arch=" + ARCH, "-o", tmp_lib] + objs + ["-lpthread"])
            for _, link in checks.values():
                if link:
                    subprocess.check_call(link)
            os.replace(tmp_lib, LIB)
            for name in checks:
                os.replace(os.path.join(work, name), check_path(name))
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


def build_check(name):
    """The device build of tests/device/<name>.hip alone (build() compiles it with the library; a host twin is compiled by the tests
    with g++): cross-compiled here, it travels with the library.  The linked kind needs the finished libcpx.so beside it."""
    if not os.path.exists(check_source(name)):
        raise RuntimeError("tests/device/%s.hip is missing: the device check cannot be built" % name)
    if CHECKS[name][1] == "linked" and not os.path.exists(LIB):
        raise RuntimeError("libcpx.so is missing: build the library first")
    os.makedirs(OUT_DIR, exist_ok=True)
    tmp = check_path(name) + ".tmp"
    try:
        for cmd in _check_cmds(name, tmp, OUT_DIR):
            if cmd:
                subprocess.check_call(cmd)
    finally:
        if os.path.exists(tmp + ".o"):
            os.remove(tmp + ".o")
    os.replace(tmp, check_path(name))
    return check_path(name)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
