"""CPU checks of the grouped verifier (cpx_batch_verify_grouped, cpx_whisk_verify_shuffle_proofs_grouped): the boundary — header, export
list, library, Rust declarations, Python wrappers, argument checks that need no device, the range of option locate_groups_max — and the
plan of the two stages (curdleproofs_amd/csrc/locate_plan.hpp), compiled with g++ into the stand-alone program
tests/host_emul/locate_plan_emul.cpp, once plain and once with -fsanitize=address,undefined, and compared with the same rules restated
here in plain Python."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.check_harness import build_emul

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("cpx_batch_verify_grouped", "cpx_whisk_verify_shuffle_proofs_grouped")
CITES = {"cpx_batch_verify_grouped": ("curdleproofs.rs:197", "msm_accumulator.rs:22-68", "curdleproofs.rs:218"),
         "cpx_whisk_verify_shuffle_proofs_grouped": ("whisk.rs:106-130",)}
OK, ERR_ARG, ERR_VERIFY, ERR_DESERIALIZE = 0, -1, -4, -5
BATCHES = (1, 2, 10, 55, 56, 255, 256, 257, 598, 600, 8192)
GROUPS_MAX = (1, 4, 255, 256)
NPT, N, FP1, FP2, SLICES = 186, 32, 4, 8, 2             # ell = 28: 4 ell + 6 + 68 points per proof, n = 32 CRS scalars; partial-sum counts as the launchers may pick them


@pytest.fixture(scope="module")
def lib():
    from curdleproofs_amd.build import build
    build()
    import curdleproofs_amd as cpx
    return cpx.load_library()


# ---- the boundary ----
def test_header_declares_both_calls_beside_their_reference_lines():
    hdr = open(os.path.join(ROOT, "include", "cpx.h")).read()
    for name in NAMES:
        at = hdr.index("int %s(" % name)
        comment = hdr[hdr.rindex("/*", 0, at):at]      # the comment block that ends right above the declaration
        for cite in CITES[name]:
            assert cite in comment, "%s: %s is not cited beside the declaration" % (name, cite)
        assert comment.rstrip().endswith("*/")
    at = hdr.index("int cpx_batch_verify_grouped(")
    comment = hdr[hdr.rindex("/*", 0, at):at]
    for words in ("Soundness", "2/r", "2^-252", '"locate_groups_max"', "n_rechecked", "drag its group into stage 2"):
        assert words in comment, words
    # the fused call now sends its callers to the grouped one
    at = hdr.index("int cpx_batch_verify_fused(")
    comment = hdr[hdr.rindex("/*", 0, at):at]
    assert "cpx_batch_verify_grouped" in comment and "re-run cpx_batch_verify " not in comment


def test_names_are_exported_everywhere(lib):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in NAMES:
        assert name in cpx.EXPORTS
        assert hasattr(lib, name), "libcpx.so does not export %s" % name
        assert re.search(r"pub fn %s\(" % name, ffi), "integration/rust/ffi.rs lacks %s" % name
    assert callable(cpx.Context.verify_batch_grouped) and callable(whisk.are_valid_whisk_shuffle_proofs_grouped)
    assert "k_vs_crs_sum_groups" in cpx.Context.KERNELS


def test_null_arguments_are_rejected_without_a_device(lib):
    import curdleproofs_amd as cpx
    buf = (ctypes.c_uint8 * 512)(*([0xaa] * 512))
    verdict = (ctypes.c_int * 2)(77, 77)
    n = ctypes.c_size_t(99)
    g, w = lib.cpx_batch_verify_grouped, lib.cpx_whisk_verify_shuffle_proofs_grouped
    # a NULL input with work to do (checked before the context is looked at), and a NULL context
    assert g(None, None, buf, verdict, ctypes.byref(n)) == cpx.CPX_ERR_ARG
    assert g(None, buf, None, verdict, ctypes.byref(n)) == cpx.CPX_ERR_ARG
    assert g(None, buf, buf, None, ctypes.byref(n)) == cpx.CPX_ERR_ARG
    assert g(None, buf, buf, verdict, ctypes.byref(n)) == cpx.CPX_ERR_ARG
    assert g(None, buf, buf, verdict, None) == cpx.CPX_ERR_ARG
    assert w(None, 1, None, buf, buf, buf, verdict, ctypes.byref(n)) == cpx.CPX_ERR_ARG
    assert w(None, 1, buf, None, buf, buf, verdict, ctypes.byref(n)) == cpx.CPX_ERR_ARG
    assert w(None, 1, buf, buf, None, buf, verdict, ctypes.byref(n)) == cpx.CPX_ERR_ARG
    assert w(None, 1, buf, buf, buf, None, verdict, ctypes.byref(n)) == cpx.CPX_ERR_ARG
    assert w(None, 1, buf, buf, buf, buf, None, ctypes.byref(n)) == cpx.CPX_ERR_ARG
    assert w(None, 1, buf, buf, buf, buf, verdict, ctypes.byref(n)) == cpx.CPX_ERR_ARG
    assert w(None, 0, None, None, None, None, None, None) == cpx.CPX_ERR_ARG          # nothing to run on, nothing written
    assert bytes(buf) == b"\xaa" * 512 and list(verdict) == [77, 77] and n.value == 99


def test_python_wrappers_check_lengths_before_touching_the_library():
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk

    class Shape:                                           # any use of the library would raise AttributeError, not ValueError
        batch, proof_size, ell = 2, 100, 4
    with pytest.raises(ValueError):
        cpx.Context.verify_batch_grouped(Shape, [bytes(100)], bytes(2 * 12 * 32))
    with pytest.raises(ValueError):
        cpx.Context.verify_batch_grouped(Shape, [bytes(100)] * 2, bytes(2 * 8 * 32))       # 12 factors per proof, not 8
    with pytest.raises(ValueError):
        whisk.are_valid_whisk_shuffle_proofs_grouped(Shape, [[None] * 4], [[None] * 4], [])
    with pytest.raises(ValueError):
        whisk.are_valid_whisk_shuffle_proofs_grouped(Shape, [[None] * 3], [[None] * 4], [b""], [bytes(12 * 32)])
    with pytest.raises(ValueError):
        whisk.are_valid_whisk_shuffle_proofs_grouped(Shape, [[None] * 4], [[None] * 4], [b""], [bytes(8 * 32)])
    assert whisk.are_valid_whisk_shuffle_proofs_grouped(Shape, [], [], []) == ([], 0)


def test_the_option_is_listed_and_bounded(lib):
    src = open(os.path.join(ROOT, "curdleproofs_amd", "csrc", "kernels.h")).read()
    assert re.search(r"long locate_groups_max = 256;", src)
    assert '{"locate_groups_max", &Options::locate_groups_max, 1, 256}' in open(os.path.join(ROOT, "curdleproofs_amd", "csrc", "kernels.hip")).read()
    assert '| `locate_groups_max` | 256 |' in open(os.path.join(ROOT, "INTEGRATION.md")).read()          # section 7's table
    # the option table itself (kernels.hip cpx::set_option / cpx::get_option on a zeroed `struct Options`: it only holds longs): no device needed
    set_option, get_option = lib._ZN3cpx10set_optionERNS_7OptionsEPKcl, lib._ZN3cpx10get_optionERKNS_7OptionsEPKcPl
    set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_long]
    set_option.restype = ctypes.c_bool
    get_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_long)]
    get_option.restype = ctypes.c_bool
    opts = ctypes.create_string_buffer(8192)
    v = ctypes.c_long(-1)
    for value, accepted in ((1, True), (256, True), (0, False), (257, False), (-1, False), (4, True)):
        assert bool(set_option(opts, b"locate_groups_max", value)) is accepted, value
        if accepted:
            assert get_option(opts, b"locate_groups_max", ctypes.byref(v)) and v.value == value
    assert get_option(opts, b"locate_groups_max", ctypes.byref(v)) and v.value == 4          # a refused value changes nothing


# ---- locate_plan.hpp on the CPU ----
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    exe = build_emul("locate_plan_emul.cpp", ["locate_plan.hpp", "include/cpx.h"], request.param == "sanitized", hip=False)

    def run(B, groups_max, flags, group_ok, own_ok):
        s = lambda bits: "".join(str(int(b)) for b in bits) or "-"
        out = subprocess.run([exe] + [str(a) for a in (B, groups_max, NPT, N, FP1, FP2, SLICES)] + [s(flags), s(group_ok), s(own_ok)], check=True, capture_output=True,
                             text=True).stdout                                             # a sanitizer report is a non-zero exit
        res = {"group": [], "stage2": []}
        for line in out.splitlines():
            key, *vals = line.split()
            vals = [int(v) for v in vals]
            if key in res:
                res[key].append(vals)
            else:
                res[key] = vals
        return res
    return run


def grouping(B, groups_max):
    """the issue's rule: G = ceil(B / locate_groups_max) proofs per group, NT = ceil(B / G) groups, the last one may be short"""
    G = -(-B // groups_max)
    return G, -(-B // G)


def patterns(B, G, NT):
    """(name, flag words, what every proof's own check says)"""
    last_first = (NT - 1) * G
    yield "no flags", [0] * B, [1] * B
    yield "every proof flagged", [1 + p % 3 for p in range(B)], [0] * B
    yield "every proof undecodable", [1] * B, [0] * B
    mid = min(G, B) // 2                                   # group 0 is always a full group
    yield "one structural flag in a full group", [2 * (p == mid) for p in range(B)], [int(p != mid) for p in range(B)]
    yield "one structural flag in the last group", [2 * (p == B - 1) for p in range(B)], [int(p != B - 1) for p in range(B)]
    yield "every group failing", [0] * B, [int(p % G != 0) for p in range(B)]
    yield "only the last group failing", [0] * B, [int(p != B - 1) for p in range(B)]
    yield "an undecodable proof beside a wrong one", [int(p == last_first) for p in range(B)], [int(p != B - 1) for p in range(B)]


def group_results(B, G, NT, flags, own):
    """stage 1 as the library computes it: an undecodable proof contributes nothing, every other proof contributes its own check value (a
    structurally rejected proof keeps its scalars, and its check does not hold)"""
    return [int(all(own[p] and not flags[p] & 2 for p in range(g * G, min((g + 1) * G, B)) if not flags[p] & 1)) for g in range(NT)]


@pytest.mark.parametrize("groups_max", GROUPS_MAX)
@pytest.mark.parametrize("B", BATCHES)
def test_plan_matches_the_rules(emul, B, groups_max):
    G, NT = grouping(B, groups_max)
    assert NT <= groups_max
    for name, flags, own in patterns(B, G, NT):
        group_ok = group_results(B, G, NT, flags, own)
        pl = emul(B, groups_max, flags, group_ok, own)
        assert pl["plan"] == [B, G, NT, int(G == 1)], name
        # the groups partition 0 .. B in order; task g starts where its first proof's points start
        assert len(pl["group"]) == NT
        nxt = 0
        for g, (idx, first, count, off, n, out_first) in enumerate(pl["group"]):
            assert idx == g and first == nxt and 1 <= count <= G and (count == G or g == NT - 1)
            assert off == first * NPT and n == count * NPT and out_first == g * FP1
            nxt += count
        assert nxt == B and pl["beyond"] == [0]
        assert pl["sizes1"] == [G * NPT, B * NPT, NT * N, 2 * NT * G * NPT, 9 * NT * G * NPT, NT * 32 * SLICES, NT * FP1, NT * 48]
        assert pl["sizes1"][3] >= 2 * B * NPT and pl["sizes1"][4] >= 9 * B * NPT            # every task's points fit the scratch
        # stage 2: the flag-free proofs of the failing groups, in batch order, dense slots; none with one proof per group
        want = [] if G == 1 else [p for p in range(B) if not flags[p] and not group_ok[p // G]]
        assert [row[1] for row in pl["stage2"]] == want, name
        for s, (idx, p, g, conv_off, out_first) in enumerate(pl["stage2"]):
            assert idx == s and g == p // G and not group_ok[g] and flags[p] == 0
            assert conv_off == s * NPT and out_first == s * FP2
            assert s == 0 or p > pl["stage2"][s - 1][1]
        S = len(want)
        assert pl["sizes2"] == [S, 2 * S * NPT, 9 * S * NPT, S * 32 * SLICES, S * FP2, S * 48]
        # verdicts
        expect = []
        for p in range(B):
            if flags[p] & 1:
                expect.append(ERR_DESERIALIZE)
            elif flags[p] & 2:
                expect.append(ERR_VERIFY)
            elif group_ok[p // G]:
                expect.append(OK)
            else:
                expect.append(OK if G > 1 and own[p] else ERR_VERIFY)
        assert pl["verdicts"] == expect, name
        # what a caller sees: exactly the per-proof verifier's verdicts
        assert expect == [ERR_DESERIALIZE if f & 1 else ERR_VERIFY if f & 2 or not o else OK for f, o in zip(flags, own)], name
        if name == "no flags":
            assert S == 0 and expect == [OK] * B
        if name == "every proof undecodable":
            assert S == 0 and group_ok == [1] * NT
        if name == "only the last group failing" and G > 1:
            assert S == B - (NT - 1) * G
        if name == "every group failing" and G > 1:
            assert S == B


def test_out_of_range_group_counts_are_clamped(emul):
    for groups_max, like in ((0, 1), (-5, 1), (257, 256), (1 << 40, 256)):
        assert emul(600, groups_max, [0] * 600, [1] * grouping(600, like)[1], [1] * 600)["plan"][:3] == [600, *grouping(600, like)]
    assert emul(0, 256, [], [], [])["plan"] == [0, 1, 0, 1]
