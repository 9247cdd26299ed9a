"""CPU checks of the grouped and the fused check of tracker proofs (cpx_whisk_verify_tracker_proofs_grouped / _fused): the boundary —
header, export list, library, Rust declarations, kernel name lists, argument checks that need no device — and the plan and scalar rules
(curdleproofs_amd/csrc/tracker_check_plan.hpp), compiled with g++ into the stand-alone program tests/host_emul/tracker_check_emul.cpp,
once plain and once with -fsanitize=address,undefined, and compared with the same rules restated here on Python integers."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from tests.check_harness import build_emul

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("cpx_whisk_verify_tracker_proofs_fused", "cpx_whisk_verify_tracker_proofs_grouped")
KERNELS = ("k_tracker_check_scalars", "k_tracker_gather")
R_ = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
COUNTS = (0, 1, 9, 37, 257, 1 << 21)
GROUPS_MAX = (1, 4, 256)
K_G, A, R_G, K_R_G, B = range(5)          # the order of an item's five points in its group's task


@pytest.fixture(scope="module")
def lib():
    from curdleproofs_amd.build import build
    build()
    import curdleproofs_amd as cpx
    return cpx.load_library()


# ---- consistency of the listings ----
def _declared_args(hdr, name):
    at = hdr.index("int %s(" % name)
    decl = hdr[at:hdr.index(";", at)]
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    return [a.strip() for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]


def test_header_export_list_library_and_rust_agree(lib):
    import curdleproofs_amd as cpx
    hdr = open(os.path.join(ROOT, "include", "cpx.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in NAMES:
        args = _declared_args(hdr, name)
        assert args[0] == "cpx_ctx* ctx" and args[1] == "size_t count"
        assert name in cpx.EXPORTS
        assert hasattr(lib, name), "libcpx.so does not export %s" % name
        assert len(getattr(lib, name).argtypes) == len(args) == 8
        assert re.search(r"pub fn %s\(" % name, ffi), "integration/rust/ffi.rs lacks %s" % name
        at = hdr.index("int %s(" % name)
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert comment.rstrip().endswith("*/")
    # the soundness statement stands beside the declarations, as the shuffle verifiers' does
    block = hdr[hdr.index("whisk.rs:183-226 for `count` triples as ONE"):hdr.index("int %s(" % NAMES[1])]
    assert "1 / r" in block and "independent" in block and "locate_groups_max" in block and "2^21" in block


def test_kernel_names_are_listed_for_the_statistics():
    import curdleproofs_amd as cpx
    hdr = open(os.path.join(ROOT, "include", "cpx.h")).read()
    names = hdr[hdr.index("name = kernel name as rocprofv3 reports it"):hdr.index("int cpx_get_stat(")]
    for k in KERNELS:
        assert k in cpx.Context.KERNELS
        assert '"%s"' % k in names
        assert not k.startswith("k_msm_")


def test_null_arguments_and_the_limit_are_rejected_without_a_device(lib):
    import curdleproofs_amd as cpx
    buf = (ctypes.c_uint8 * 144)()
    st = (ctypes.c_int * 1)(7)
    n = ctypes.c_size_t(5)
    inv = ctypes.c_int(9)
    for missing in range(4):
        args = [buf, buf, buf, buf]
        args[missing] = None
        assert lib.cpx_whisk_verify_tracker_proofs_grouped(None, 1, *args, st, ctypes.byref(n)) == cpx.CPX_ERR_ARG
        assert lib.cpx_whisk_verify_tracker_proofs_fused(None, 1, *args, buf, ctypes.byref(inv)) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_verify_tracker_proofs_grouped(None, 1, buf, buf, buf, buf, None, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_verify_tracker_proofs_fused(None, 1, buf, buf, buf, buf, None, ctypes.byref(inv)) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_verify_tracker_proofs_fused(None, 1, buf, buf, buf, buf, buf, None) == cpx.CPX_ERR_ARG
    # one more than 2^21 items: refused before a buffer (here: one far too small) or the context is looked at
    assert lib.cpx_whisk_verify_tracker_proofs_grouped(None, (1 << 21) + 1, buf, buf, buf, buf, st, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_verify_tracker_proofs_fused(None, (1 << 21) + 1, buf, buf, buf, buf, buf, ctypes.byref(inv)) == cpx.CPX_ERR_ARG
    # a NULL context with well-formed arguments
    assert lib.cpx_whisk_verify_tracker_proofs_grouped(None, 1, buf, buf, buf, buf, st, None) == cpx.CPX_ERR_ARG
    assert st[0] == 7 and n.value == 5 and inv.value == 9 and bytes(buf) == bytes(144)


def test_python_wrappers_check_lengths_before_touching_the_library():
    from curdleproofs_amd import whisk
    t = whisk.WhiskTracker(b"\x01" * 48, b"\x02" * 48)
    ctx = None                                             # any use of the context would raise AttributeError, not ValueError
    for f in (whisk.are_valid_whisk_tracker_proofs_grouped, whisk.whisk_tracker_proofs_partial, whisk.are_all_valid_whisk_tracker_proofs):
        with pytest.raises(ValueError):
            f(ctx, [t, t], [bytes(48)], [bytes(128), bytes(128)])
        with pytest.raises(ValueError):
            f(ctx, [t], [bytes(48)], [bytes(128)], rands=[])
        with pytest.raises(ValueError):
            f(ctx, [t], [bytes(48)], [bytes(128)], rands=[bytes(32)])
    assert whisk.are_valid_whisk_tracker_proofs_grouped(ctx, [], [], []) == ([], 0)


# ---- the g++ twin of tracker_check_plan.hpp ----
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    exe = build_emul("tracker_check_emul.cpp", ["include/cpx.h", "tracker_check_plan.hpp", "locate_plan.hpp", "mont32.hpp"], request.param == "sanitized", hip=False)

    def run(args, stdin=None):
        return subprocess.run([exe] + [str(a) for a in args], input=stdin, check=True, capture_output=True, text=True).stdout   # a sanitizer report is a non-zero exit
    return run


def _grouping(count, groups_max):
    """locate_plan restated: (items per group, groups)"""
    gm = min(max(groups_max, 1), 256)
    G = -(-count // gm) if count else 1
    return G, -(-count // G)


@pytest.mark.parametrize("groups_max", GROUPS_MAX)
@pytest.mark.parametrize("count", COUNTS)
def test_task_layout_matches_python_integers(emul, count, groups_max):
    G, NT = _grouping(count, groups_max)
    lines = emul(["plan", count, groups_max]).splitlines()
    assert lines[0].split() == ["plan", str(count), str(G), str(NT), "1"]
    groups = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("group")]
    assert len(groups) == NT
    want_off = 0
    for g, (gi, first, n, off, tn, gen_slot) in enumerate(groups):
        assert (gi, first) == (g, g * G)
        assert n == min(G, count - g * G) and n >= 1
        assert off == want_off == gen_slot and tn == 1 + 5 * n          # the tasks lie one behind the other, the generator first
        want_off += tn
    if count:
        assert groups[-1][2] == count - (NT - 1) * G                    # the last group may be short
        assert (groups[-1][2] < G) == (count % G != 0)
    sizes = [int(x) for x in next(ln for ln in lines if ln.startswith("sizes")).split()[1:]]
    assert sizes == [1 + 5 * G if count else 0, NT + 5 * count, 272 * count, 2 * count, NT, 1 << 21]
    assert want_off == NT + 5 * count <= (1 << 24)
    assert next(ln for ln in lines if ln.startswith("planes")).split()[1:] == ["4", "0", "3", "2", "1"]   # k_decompress leaves A, B, k_r_G, r_G, k_G
    layout = [int(x) for x in next(ln for ln in lines if ln.startswith("layout")).split()[1:]]
    assert layout[:4] == [0, 96 * count, 144 * count, 272 * count]           # trackers | k_commitments | proofs
    assert list(zip(layout[4::2], layout[5::2])) == [(144 * count, 128), (144 * count + 48, 128), (48, 96), (0, 96), (96 * count, 48)]
    if not count:
        return
    # slots: every item of a small batch, the first and last item of every group of a large one
    items = list(range(count)) if count <= 257 else sorted({p for g in range(NT) for p in (g * G, min(count, (g + 1) * G) - 1)})
    out = emul(["slots", count, groups_max] + items).splitlines()
    seen = set()
    for p, ln in zip(items, out):
        got = [int(x) for x in ln.split()[1:]]
        g = p // G
        base = groups[g][3] + 1 + 5 * (p - g * G)
        assert got == [p] + [base + j for j in range(5)]
        assert groups[g][3] < got[1] and got[5] < groups[g][3] + groups[g][4]      # inside its own task, behind the generator
        assert not seen & set(got[1:])                                             # no two items share a slot
        seen |= set(got[1:])
    if count <= 257:
        assert seen | {gr[3] for gr in groups} == set(range(NT + 5 * count))       # and every slot has exactly one owner


def test_the_limit_is_where_the_header_says(emul):
    assert emul(["plan", (1 << 21) + 1, 256]).splitlines()[0].split()[-1] == "0"
    assert 5 * (1 << 21) + 256 <= 1 << 24 < 5 * (1 << 22)


def _hex(v):
    return "%064x" % v


def _scalars(emul, quads):
    out = emul(["scalars"], stdin="".join(" ".join(_hex(v) for v in q) + "\n" for q in quads)).splitlines()
    assert len(out) == len(quads)
    return [[int(x, 16) for x in ln.split()] for ln in out]


def test_scalar_rules_match_python_integers(emul):
    rnd = random.Random(2024)
    edge = [0, 1, R_ - 1]
    quads = [(a, b, s, c) for a in edge for b in edge for s in edge for c in edge] + [tuple(rnd.randrange(R_) for _ in range(4)) for _ in range(64)]
    for (a, b, s, c), got in zip(quads, _scalars(emul, quads)):
        want = [a * c % R_, -a % R_, b * s % R_, b * c % R_, -b % R_, a * s % R_]
        assert got == want, (a, b, s, c)
        assert all(0 <= v < R_ for v in got)                                       # reduced, also - 0 = 0


def test_signs_without_a_curve(emul):
    """Every point stands in for its discrete log: G = 1, k_G = k, r_G = r, k_r_G = k r, A = beta, B = beta r, s = beta - c k.  The scalars of
    the twin times these logs (plus the generator term) sum to 0 for a valid item, to a delta / b delta when the claimed A / B falls short of the relation's left side by delta."""
    rnd = random.Random(77)
    cases = []
    for _ in range(32):
        k, r, beta, c, a, b = (rnd.randrange(1, R_) for _ in range(6))
        cases.append((k, r, beta, c, a, b))
    cases += [(0, 5, 7, 11, 13, 17), (1, 1, 0, R_ - 1, R_ - 1, 1), (R_ - 1, R_ - 1, R_ - 1, 1, 1, R_ - 1)]   # k = 0, blinder = 0, r = 1, extremes
    quads = [(a, b, (beta - c * k) % R_, c) for k, r, beta, c, a, b in cases]
    for (k, r, beta, c, a, b), got in zip(cases, _scalars(emul, quads)):
        def total(dA=0, dB=0):
            logs = {K_G: k, A: (beta - dA) % R_, R_G: r, K_R_G: k * r % R_, B: (beta * r - dB) % R_}
            return (got[5] + sum(got[j] * logs[j] for j in range(5))) % R_
        delta = rnd.randrange(1, R_)
        assert total() == 0
        # the item's value is a (s G + c k_G - A) + b (s r_G + c k_r_G - B)
        assert total(dA=delta) == a * delta % R_ != 0
        assert total(dB=delta) == b * delta % R_ != 0
        assert total(dA=delta, dB=delta) == (a + b) * delta % R_
