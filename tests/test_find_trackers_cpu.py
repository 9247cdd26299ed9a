"""CPU checks of cpx_whisk_find_trackers: the boundary — header, export list, library, Rust declarations, argument checks that need no
device — and curdleproofs_amd/csrc/find_plan.hpp compiled with g++: the plan (tests/host_emul/find_plan_emul.cpp: path choice, chunking
under a memory budget, the wave map, the limits) and the per-pair body of the scan (tests/host_emul/find_scan_emul.cpp) on a table the
emulation builds with the one-lane host formulas, compared with Python integers and the oracle."""
import ctypes
import os
import re
import subprocess

import pytest

from tests import find_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "curdleproofs_amd", "csrc")
NAME = "cpx_whisk_find_trackers"
KERNELS = ("k_find_scan", "k_find_compare")
FR, AFF = 32, 96
MIN_KEYS_MAX = (1 << 20) + 1
COL_BYTES = 32 * 128 * 128          # one tracker's table: 32 windows x 128 multiples x one 128-byte line


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def _deps(src):
    return [src] + [os.path.join(CSRC, f) for f in ("find_plan.hpp", "recode.hpp", "glv.hpp", "g1_28.hpp", "fp28.hpp", "g1.hpp", "mont32.hpp")]


@pytest.fixture(scope="module")
def lib():
    from curdleproofs_amd.build import build
    build()
    import curdleproofs_amd as cpx
    return cpx.load_library()


@pytest.fixture(scope="module")
def plan_exe():
    src = os.path.join(HERE, "host_emul", "find_plan_emul.cpp")
    exe = os.path.join(HERE, "host_emul", "_find_plan")
    if _stale(exe, _deps(src)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, src])
    return exe


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
    res, chunks = {}, []
    for line in out.splitlines():
        key, *vals = line.split()
        if key == "chunk":
            chunks.append(dict(zip(("index", "first", "cols", "bytes", "table_entries", "shift_entries", "tmp_entries", "waves"), map(int, vals))))
        else:
            res[key] = int(vals[0])
    res["chunks"] = chunks
    return res


@pytest.fixture(scope="module")
def emul():
    src = os.path.join(HERE, "host_emul", "find_scan_emul.cpp")
    so = os.path.join(HERE, "host_emul", "_find_scan.so")
    if _stale(so, _deps(src)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    L.emul_find_consts.argtypes = [vp]
    L.emul_find_digits.argtypes = [ci, vp, vp]
    L.emul_find_entry.argtypes = [ci, ci, cl, cl]
    L.emul_find_entry.restype = cl
    L.emul_find_build.argtypes = [ci, vp]
    L.emul_find_table_entry.argtypes = [cl, vp]
    L.emul_find_pairs.argtypes = [ci, vp, vp, vp, vp]
    for f in (L.emul_find_consts, L.emul_find_digits, L.emul_find_build, L.emul_find_table_entry, L.emul_find_pairs):
        f.restype = None
    return L


# ---- the boundary ----
def test_header_declares_the_call_beside_its_reference_lines():
    hdr = open(os.path.join(ROOT, "include", "cpx.h")).read()
    at = hdr.index("int %s(" % NAME)
    comment = hdr[hdr.rindex("/*", 0, at):at]
    assert "whisk.rs:36-55" in comment and "whisk.rs:323" in comment and comment.rstrip().endswith("*/")
    assert re.search(r"#define CPX_NO_OWNER 0xffffffffu", hdr)
    for k in KERNELS:
        assert '"%s"' % k in hdr, "cpx_get_stat's comment does not list %s" % k
    # the two consequences of the relation, the limits and the options are said where the call is declared
    for words in ("EVERY key", "duplicate keys", "2^23", "2^20", "2^32", '"find_table_min_keys"', '"find_table_mb"', "NOT rejected", "ONE stream synchronisation"):
        assert words in hdr, words


def test_name_is_exported_everywhere(lib):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "whisk_mi355x.rs")).read()
    assert NAME in cpx.EXPORTS and hasattr(lib, NAME)
    assert re.search(r"pub fn %s\(" % NAME, ffi) and "pub const CPX_NO_OWNER: u32 = 0xffff_ffff;" in ffi
    assert re.search(r"pub fn find_whisk_trackers\(trackers: &\[WhiskTracker\], ks: &\[Fr\]\) -> Vec<Result<Option<usize>, SerializationError>>", rs)
    assert NAME + "(" in rs
    for k in KERNELS:
        assert k in cpx.Context.KERNELS and not k.startswith("k_msm_")
    assert callable(whisk.find_trackers) and cpx.CPX_NO_OWNER == 0xffffffff
    assert "find.hip" in open(os.path.join(ROOT, "curdleproofs_amd", "build.py")).read()


def test_null_and_over_limit_arguments_are_rejected_without_a_device(lib):
    import curdleproofs_amd as cpx
    trk = (ctypes.c_uint8 * 96)(*([0xaa] * 96))
    key = (ctypes.c_uint8 * 32)(*([0xaa] * 32))
    owner = (ctypes.c_uint32 * 1)(0x55555555)
    status = (ctypes.c_int * 1)(77)
    f = lib.cpx_whisk_find_trackers
    assert f(None, 1, None, 1, key, owner, status) == cpx.CPX_ERR_ARG
    assert f(None, 1, trk, 1, None, owner, status) == cpx.CPX_ERR_ARG
    assert f(None, 1, trk, 1, key, None, status) == cpx.CPX_ERR_ARG
    assert f(None, 1, trk, 1, key, owner, None) == cpx.CPX_ERR_ARG
    assert f(None, 1, trk, 1, key, owner, status) == cpx.CPX_ERR_ARG                     # a NULL context
    assert f(None, 0, None, 0, None, None, None) == cpx.CPX_ERR_ARG                      # ... also for the no-op
    # beyond the limits nothing is read: the one-tracker buffers stand in for arrays that do not exist
    for n, nk in (((1 << 23) + 1, 1), (1, (1 << 20) + 1), (1 << 23, 1 << 10), ((1 << 12) + 1, 1 << 20)):
        assert f(None, n, trk, nk, key, owner, status) == cpx.CPX_ERR_ARG, (n, nk)
    assert bytes(trk) == b"\xaa" * 96 and owner[0] == 0x55555555 and status[0] == 77    # nothing was written


def test_python_wrapper_checks_lengths_before_touching_the_library():
    from curdleproofs_amd import whisk
    ctx = None                                             # any use of the context would raise AttributeError, not ValueError
    t = whisk.WhiskTracker(bytes(48), bytes(48))
    with pytest.raises(ValueError):
        whisk.find_trackers(ctx, [t], [bytes(31)])
    with pytest.raises(ValueError):
        whisk.find_trackers(ctx, [t], [bytes(32), bytes(33)])
    with pytest.raises(ValueError):
        whisk.find_trackers(ctx, [t] * 4097, [bytes(32)] * (1 << 20))          # 2^32 + 2^20 pairs
    assert whisk.find_trackers(ctx, [], []) == ([], []) and whisk.find_trackers(ctx, [], [bytes(32)]) == ([], [])


def test_options_exist_with_their_ranges(lib):
    src = open(os.path.join(CSRC, "kernels.h")).read()
    assert re.search(r"long find_table_min_keys = \d+;", src) and "long find_table_mb = 1024;" in src
    assert "profiles/find_trackers.md" in src[src.index("long find_table_min_keys"):src.index("long find_table_mb")]
    hip = open(os.path.join(CSRC, "kernels.hip")).read()
    assert '{"find_table_min_keys", &Options::find_table_min_keys, 1, (1L << 20) + 1}' in hip
    assert '{"find_table_mb", &Options::find_table_mb, 1, 65536}' in hip


# ---- the plan ----
SHAPES = ((1, 1), (63, 1), (64, 2), (65, 3), (70, 5))


@pytest.mark.parametrize("n,nk", SHAPES)
def test_plan_covers_every_pair_once(plan_exe, n, nk):
    p = _run(plan_exe, "plan", n, nk, 1, 1024)
    assert p["table"] == 1 and p["n_chunks"] == 1 and p["chunk_cols"] == n
    assert p["pairs"] == n * nk == p["pairs_taken_once"] and p["lanes_out_of_range"] == 0 and p["columns"] == n
    c = p["chunks"][0]
    assert c["waves"] == nk * ((n + 63) // 64)                                         # one wave per (key, 64 consecutive columns)
    assert c["table_entries"] == 32 * 128 * n and c["shift_entries"] == 32 * n
    assert c["tmp_entries"] >= max(31 * n, 32 * n * p["fix_chunk"])                    # what k_table_build and k_fix_build write
    assert c["bytes"] <= 1024 << 20


@pytest.mark.parametrize("mb,cols", [(1, 1), (2, 3), (3, 5)])
def test_plan_chunks_by_memory(plan_exe, mb, cols):
    """9 trackers x 64 keys under a budget of a few MiB: a column's table alone is 0.5 MiB, so 1 MiB holds one column with its build scratch,
    3 MiB five — chunks of 5 and 4, a short last one"""
    p = _run(plan_exe, "plan", 9, 64, 64, mb)
    assert p["table"] == 1 and p["chunk_cols"] == cols and p["n_chunks"] == -(-9 // cols)
    assert [c["cols"] for c in p["chunks"]] == [cols] * (9 // cols) + ([9 % cols] if 9 % cols else [])
    assert [c["first"] for c in p["chunks"]] == [cols * i for i in range(p["n_chunks"])]
    for c in p["chunks"]:
        assert c["bytes"] <= mb << 20 and c["table_entries"] * 128 == COL_BYTES * c["cols"]
        assert c["bytes"] == c["table_entries"] * 128 + c["shift_entries"] * 112 + c["tmp_entries"] * 224
        assert c["tmp_entries"] * 224 * 4 <= c["table_entries"] * 128                   # the scratch does not dominate
        assert c["waves"] == 64
    assert p["next_bytes"] > mb << 20                                                   # one more column would not fit
    assert 128 % p["fix_chunk"] == 0 and p["fix_chunk"] >= 1                            # k_fix_build walks 128 multiples in whole rounds
    assert p["pairs_taken_once"] == 9 * 64 == p["pairs"] and p["lanes_out_of_range"] == 0


def test_plan_default_budget_keeps_whole_waves(plan_exe):
    p = _run(plan_exe, "plan", 8192, 2, 1, 1024)
    assert p["chunk_cols"] % 64 == 0 and p["chunk_cols"] * COL_BYTES <= 1024 << 20 < (p["chunk_cols"] + 64) * (COL_BYTES + 60000)
    assert sum(c["cols"] for c in p["chunks"]) == 8192 and p["chunks"][-1]["cols"] <= p["chunk_cols"]
    assert all(c["bytes"] <= 1024 << 20 for c in p["chunks"])
    assert p["pairs_taken_once"] == 8192 * 2 and p["lanes_out_of_range"] == 0


@pytest.mark.parametrize("min_keys", [1, 2, 64, 1 << 20, MIN_KEYS_MAX])
def test_path_choice_sits_at_the_threshold(plan_exe, min_keys):
    for nk in (min_keys - 1, min_keys, min_keys + 1):
        if nk < 0 or nk > 1 << 20:
            continue
        p = _run(plan_exe, "plan", 3, nk, min_keys, 1024)
        assert p["table"] == int(nk >= min_keys and nk > 0), (nk, min_keys)
    assert _run(plan_exe, "plan", 0, 5, 1, 1024)["table"] == 0                          # nothing to do


def test_limits(plan_exe):
    fits = lambda n, nk: _run(plan_exe, "fits", n, nk)["fits"]
    assert fits(1 << 23, 1 << 9) == 1 and fits((1 << 23) + 1, 1) == 0
    assert fits(1 << 12, 1 << 20) == 1 and fits(1, (1 << 20) + 1) == 0
    assert fits(1 << 16, 1 << 16) == 1 and fits((1 << 16) + 1, 1 << 16) == 0 and fits(1 << 23, (1 << 9) + 1) == 0
    assert fits(0, 0) == 1 and fits(1 << 23, 0) == 1


# ---- the key sets ----
def test_coverage_set_reaches_every_attainable_pick():
    want = fc.attainable_picks()
    assert len(want) == 31 * 255 + 0x74 and fc.top_digit_max() == 0x74                  # r - 1 gives 0x74
    assert fc.picks_of(fc.coverage_keys()) == want
    assert (31, 0x74, 0) in fc.picks_of([fc.R_ - 1]) and (0, 128, 1) in want and (0, 128, 0) not in want
    keys = fc.coverage_keys() + [k for k in fc.edge_keys() if k not in set(fc.coverage_keys())]
    assert len(set(keys)) == len(keys) and all(0 <= k < fc.R_ for k in keys)           # distinct mod r
    e = fc.edge_keys()
    for v in (0, 1, fc.R_ - 1, 1 << 8, (1 << 8) - 1, 1 << 248, (1 << 248) - 1, int.from_bytes(b"\x80" * 31, "little"), int.from_bytes(b"\x7f" * 31, "little")):
        assert v in e
    assert [-128] + [-127] * 30 + [1] == fc.signed_digits(int.from_bytes(b"\x80" * 31, "little"))       # both ends of the carries
    assert [127] * 31 + [0] == fc.signed_digits(int.from_bytes(b"\x7f" * 31, "little"))


def test_twin_digits_and_entries_match_python(emul):
    c = (ctypes.c_int * 4)()
    emul.emul_find_consts(c)
    assert list(c) == [32, 128, 64, 128]
    keys = fc.edge_keys() + fc.coverage_keys()
    d = (ctypes.c_int * (32 * len(keys)))()
    emul.emul_find_digits(len(keys), fc.to_bytes(keys), d)
    for j, k in enumerate(keys):
        assert list(d[32 * j:32 * (j + 1)]) == fc.signed_digits(k), hex(k)
    for w, dd, nc, col in ((0, 1, 1, 0), (31, 0x74, 7, 6), (5, -128, 70, 69), (30, 127, 1792, 1000)):
        assert emul.emul_find_entry(w, dd, nc, col) == (w * 128 + abs(dd) - 1) * nc + col


# ---- the per-pair body on a table built by the twin ----
def test_scan_body_on_the_cpu_matches_the_oracle(emul, orc):
    fr = lambda v: orc.fr_from_canonical_bytes((v % fc.R_).to_bytes(32, "little"))
    gen = orc.g1_generator()
    other = orc.g1_scale(gen, fr(0x1234567890abcdef1234567890abcdef))
    ident = bytes(AFF)
    bases = [gen, other, ident]
    nc = len(bases)
    emul.emul_find_build(nc, b"".join(bases))
    # the table itself: the last multiple of a few windows against the oracle
    for col, base in enumerate(bases[:2]):
        for w, m in ((0, 1), (0, 128), (7, 128), (31, 0x74)):
            out = ctypes.create_string_buffer(AFF)
            emul.emul_find_table_entry(emul.emul_find_entry(w, m, nc, col), out)
            assert out.raw == orc.g1_scale(base, fr(m * 256 ** w)), (col, w, m)
    keys = fc.edge_keys() + fc.coverage_keys()[::4]
    assert len(fc.coverage_keys()[::4]) == 64
    nk = len(keys)
    true = [[orc.g1_scale(b, fr(k)) for b in bases] for k in keys]                      # every (key, base) product from the oracle
    neg = lambda aff: orc.g1_scale(aff, fr(fc.R_ - 1))
    ok = bytes([1] * nc)
    expect_same = lambda got, want: orc.g1_compress(got) == orc.g1_compress(want)

    def run(claimed, ok_flags=ok):
        m = (ctypes.c_int * (nk * nc))()
        emul.emul_find_pairs(nk, fc.to_bytes(keys), b"".join(claimed[j][c] for j in range(nk) for c in range(nc)), ok_flags, m)
        return [[m[j * nc + c] for c in range(nc)] for j in range(nk)]

    # the true products: every pair matches (the identity base against the identity claim included)
    assert run(true) == [[1] * nc for _ in keys]
    # the negated product: no match, except where the product is the identity (key 0, or the identity base)
    got = run([[neg(p) for p in row] for row in true])
    for j, k in enumerate(keys):
        for c in range(nc):
            assert got[j][c] == int(expect_same(neg(true[j][c]), true[j][c])), (hex(k), c)
    assert got[keys.index(1)][0] == 0 and got[keys.index(0)][0] == 1 and got[keys.index(1)][2] == 1
    # the next key's product, the other base's product, and a claim against the identity base that is not the identity
    shifted = [[true[(j + 1) % nk][c] for c in range(nc)] for j in range(nk)]
    got = run(shifted)
    for j in range(nk):
        for c in range(nc):
            assert got[j][c] == int(expect_same(shifted[j][c], true[j][c])), (j, c)
    swapped = [[true[j][1], true[j][0], gen] for j in range(nk)]
    got = run(swapped)
    for j in range(nk):
        assert got[j] == [int(expect_same(true[j][1], true[j][0])), int(expect_same(true[j][0], true[j][1])), 0], j
    # a tracker that did not decode never matches, whatever its (identity) points say
    assert run(true, bytes([1, 1, 0])) == [[1, 1, 0] for _ in keys]
