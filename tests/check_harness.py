"""The Python side of tests/device/check_harness.hpp, shared by the libraries of the seven check programs (field_check_lib,
scalar_check_lib, rng_cases, rng_g1_cases, transcript_cases, msm_check_lib, quad_check_lib): building a host twin, the record file format, running a
program over a record file and the bit-for-bit comparison.  build_emul() compiles the CPU twins of the plan headers
(tests/host_emul/*_emul.cpp) for the tests/test_*_cpu.py files."""
import os
import shutil
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = "<48sIIQ"        # name, words per row, reserved, rows (tests/device/check_harness.hpp)


def build_host_twin(src, out_dir, name, extra=()):
    """the host twin of a check program: the same source through g++ as plain C++"""
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call(["g++", "-x", "c++", "-O2", "-std=c++17"] + list(extra) + ["-o", exe, src])
    return exe


def list_operations(exe):
    """--list as {name: (input words, output words)}, or {name: group} for the two-column form of msm_check"""
    out = subprocess.run([exe, "--list"], capture_output=True, text=True, timeout=120, check=True).stdout
    rows = [l.split() for l in out.splitlines()]
    return {r[0]: r[1] if len(r) == 2 else (int(r[1]), int(r[2])) for r in rows}


def pack_record(name, width, rows, payload):      # (HEADER spelled out: the one writer of the format, where a search for it lands)
    return struct.pack("<48sIIQ", name.encode(), width, 0, rows) + payload


def pack_records(table, records):
    """records: list of (operation, rows) with every row a flat list of integers in [-2^31, 2^32); table[operation][0] is the row width"""
    out = []
    for name, rows in records:
        ni = table[name][0]
        a = np.array(rows, dtype=np.int64).reshape(len(rows), ni)
        assert a.min(initial=0) >= -(1 << 31) and a.max(initial=0) < (1 << 32), name
        out.append(pack_record(name, ni, len(rows), (a & 0xffffffff).astype("<u4").tobytes()))
    return b"".join(out)


def write_records(path, table, records):
    with open(path, "wb") as f:
        f.write(pack_records(table, records))


def read_records(path):
    """list of (operation, array rows x words, uint32)"""
    out = []
    with open(path, "rb") as f:
        data = f.read()
    o = 0
    while o < len(data):
        name, words, _, rows = struct.unpack_from(HEADER, data, o)
        o += 64
        a = np.frombuffer(data, dtype="<u4", count=rows * words, offset=o).reshape(rows, words)
        o += 4 * rows * words
        out.append((name.rstrip(b"\0").decode(), a))
    return out


def run_file(exe, data, work_dir, tag, timeout, summary):
    """one process: `exe` over the record file `data`; it must exit 0 and print `summary`.  Returns the path of the output file."""
    inp, outp = os.path.join(str(work_dir), tag + ".in"), os.path.join(str(work_dir), tag + ".out")
    with open(inp, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "%s exited with %d: %s" % (os.path.basename(exe), r.returncode, (r.stdout + r.stderr)[-2000:])
    assert summary in r.stdout, r.stdout
    return outp


def run(exe, table, records, work_dir, tag, timeout=120):
    """one process: every record through `exe`; the outputs in order, one per record, names, shapes and the summary line checked"""
    summary = "%d records, %d rows" % (len(records), sum(len(r) for _, r in records))
    res = read_records(run_file(exe, pack_records(table, records), work_dir, tag, timeout, summary))
    assert [n for n, _ in res] == [n for n, _ in records]
    for (name, rows), (_, a) in zip(records, res):
        assert a.shape == (len(rows), table[name][1]), name
    return res


def _fmt(row):
    return "[" + ", ".join(hex(x) if x >= 0 else "-" + hex(-x) for x in row) + "]"


def assert_same(records, got, want, who=("device", "host twin")):
    """bit for bit, every row of every record; returns the number of rows compared"""
    n = 0
    for (name, rows), (_, g), (_, w) in zip(records, got, want):
        assert g.shape == w.shape, name
        if not np.array_equal(g, w):
            i = int(np.nonzero((g != w).any(axis=1))[0][0])
            raise AssertionError("%s row %d: %s and %s differ\n  in  %s\n  %s %s\n  %s %s" % (
                name, i, who[0], who[1], _fmt(rows[i]), who[0], _fmt(g[i].tolist()), who[1], _fmt(w[i].tolist())))
        n += len(rows)
    return n


# ---------------------------------------------------------------- the CPU twins of the plan headers

def hip_include():
    """the include directory of the HIP headers: the planners make no HIP call, but kernels.h and protocol.h include hip_runtime.h"""
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(c))), "include")
    raise RuntimeError("the HIP headers were not found")


def build_emul(src, deps, sanitized=False, hip=True, shared=False):
    """Compiles `src` = tests/host_emul/<name>_emul.cpp with g++ to tests/host_emul/_<name>[_san] if that is missing or older than the
    source or one of `deps` (a bare name: a file of curdleproofs_amd/csrc; else a path from the repository's root), and returns its
    path.  The line is -std=c++17 -Wall -Wextra -Werror, then -O2 or (sanitized) -O1 -g -fsanitize=address,undefined
    -fno-sanitize-recover=all, then (hip) -D__HIP_PLATFORM_AMD__ -isystem <hip include>.  A sanitized build is a stand-alone program:
    its report is a non-zero exit of that program.  shared: the two planners that a test calls through ctypes, _<name>.so with the
    line they have always had (-O1 -std=c++17 -fPIC -shared -D__HIP_PLATFORM_AMD__ -I <hip include>), never sanitized."""
    src = os.path.join(HERE, "host_emul", src)
    out = os.path.join(HERE, "host_emul", "_" + os.path.basename(src)[:-len("_emul.cpp")] + ("_san" if sanitized else "") + (".so" if shared else ""))
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + [os.path.join(ROOT, d if "/" in d else "curdleproofs_amd/csrc/" + d) for d in deps]):
        if shared:
            flags = ["-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I", hip_include()]
        else:
            flags = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
            flags += ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
            flags += ["-D__HIP_PLATFORM_AMD__", "-isystem", hip_include()] if hip else []
        subprocess.check_call(["g++"] + flags + ["-o", out, src])
    return out
