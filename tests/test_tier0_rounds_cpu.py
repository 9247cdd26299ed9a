"""CPU checks of the per-round tier-0 calls (cpx_g1_msm_many, cpx_g1_fold_many): the boundary — header, export list, library, Rust
declarations, argument checks that need no device, the Python wrappers' shape errors — and the offset and size arithmetic of the calls
(curdleproofs_amd/csrc/tier0_plan.hpp), compiled with g++ into the stand-alone program tests/host_emul/tier0_plan_emul.cpp, once plain
and once with -fsanitize=address,undefined, and compared with the layout restated here in plain Python."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.check_harness import build_emul

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("cpx_g1_msm_many", "cpx_g1_fold_many")
CITES = {"cpx_g1_msm_many": ("util.rs:19-22", "inner_product_argument.rs:158-161", "same_multiscalar_argument.rs:107-112"),
         "cpx_g1_fold_many": ("inner_product_argument.rs:177-178", "same_multiscalar_argument.rs:128-130")}
RAGGED = (0, 1, 2, 15, 16, 17, 63, 64, 65, 129)
# the length lists of tests/test_gpu_tier0_rounds.py
LENGTH_LISTS = (RAGGED, RAGGED[::-1], (64,) * 6, (129, 128, 129, 128), (7,), (0,), (3,) * 40, (1030, 5, 0, 64), (16,), (1024,) * 16, (1024,) * 17, (511,), (512,),
                (1023,), (2048, 1), (255,) * 32, (300,) * 33, ())


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
    assert '"fold_quad_max"' in hdr and "scripts/tier0_round_timing.py" in hdr          # the option and where the cost is measured


def test_names_are_exported_everywhere(lib):
    import curdleproofs_amd as cpx
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in NAMES:
        assert name in cpx.EXPORTS
        assert hasattr(lib, name), "libcpx.so does not export %s" % name
        assert re.search(r"pub fn %s\(" % name, ffi), "integration/rust/ffi.rs lacks %s" % name
    assert callable(cpx.Context.msm_many) and callable(cpx.Context.fold_many)


def test_null_arguments_are_rejected_without_a_device(lib):
    import curdleproofs_amd as cpx
    buf = (ctypes.c_uint8 * 288)(*([0xaa] * 288))
    lens = (ctypes.c_uint32 * 1)(1)
    # a NULL input with work to do (checked before the context is looked at), and a NULL context
    assert lib.cpx_g1_msm_many(None, 1, None, buf, buf, buf, buf) == cpx.CPX_ERR_ARG
    assert lib.cpx_g1_msm_many(None, 1, lens, None, buf, buf, buf) == cpx.CPX_ERR_ARG
    assert lib.cpx_g1_msm_many(None, 1, lens, buf, None, buf, buf) == cpx.CPX_ERR_ARG
    assert lib.cpx_g1_msm_many(None, 1, lens, buf, buf, buf, buf) == cpx.CPX_ERR_ARG
    assert lib.cpx_g1_msm_many(None, 0, None, None, None, None, None) == cpx.CPX_ERR_ARG       # nothing to run on, nothing written
    assert lib.cpx_g1_fold_many(None, 1, 1, None, buf, buf) == cpx.CPX_ERR_ARG
    assert lib.cpx_g1_fold_many(None, 1, 1, buf, None, buf) == cpx.CPX_ERR_ARG
    assert lib.cpx_g1_fold_many(None, 1, 1, buf, buf, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_g1_fold_many(None, 1, 1, buf, buf, buf) == cpx.CPX_ERR_ARG
    assert lib.cpx_g1_fold_many(None, 0, 0, None, None, None) == cpx.CPX_ERR_ARG
    assert bytes(buf) == b"\xaa" * 288 and lens[0] == 1


def test_python_wrappers_check_lengths_before_touching_the_library():
    import curdleproofs_amd as cpx
    ctx = None                                             # any use of the context would raise AttributeError, not ValueError
    with pytest.raises(ValueError):
        cpx.Context.msm_many(ctx, [bytes(96)], [])
    with pytest.raises(ValueError):
        cpx.Context.msm_many(ctx, [bytes(96)], [bytes(64)])
    with pytest.raises(ValueError):
        cpx.Context.msm_many(ctx, [bytes(96), bytes(95)], [bytes(32), bytes(32)])
    with pytest.raises(ValueError):
        cpx.Context.fold_many(ctx, [bytes(96)], [bytes(96), bytes(96)], [bytes(32)])
    with pytest.raises(ValueError):
        cpx.Context.fold_many(ctx, [bytes(96), bytes(192)], [bytes(96), bytes(192)], [bytes(32)] * 2)
    with pytest.raises(ValueError):
        cpx.Context.fold_many(ctx, [bytes(96)], [bytes(192)], [bytes(32)])
    with pytest.raises(ValueError):
        cpx.Context.fold_many(ctx, [bytes(96)], [bytes(96)], [bytes(31)])
    with pytest.raises(ValueError):
        cpx.Context.fold_many(ctx, [bytes(96)], [bytes(96)], bytes(64))
    assert cpx.Context.msm_many(ctx, [], []) == [] and cpx.Context.msm_many(ctx, [], [], compressed=True) == ([], [])
    assert cpx.Context.fold_many(ctx, [], [], []) == []


def test_the_option_is_listed_beside_the_others():
    src = open(os.path.join(ROOT, "curdleproofs_amd", "csrc", "kernels.h")).read()
    assert re.search(r"long fold_quad_max = \d+;", src)
    assert '{"fold_quad_max", &Options::fold_quad_max, 0,' in open(os.path.join(ROOT, "curdleproofs_amd", "csrc", "kernels.hip")).read()


# ---- tier0_plan.hpp on the CPU ----
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    exe = build_emul("tier0_plan_emul.cpp", ["tier0_plan.hpp"], request.param == "sanitized", hip=False)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout       # a sanitizer report is a non-zero exit
        res = {"task": []}
        for line in out.splitlines():
            key, *vals = line.split()
            vals = [int(v) for v in vals]
            if key == "task":
                res["task"].append(vals)
            else:
                res[key] = vals[0]
        return res
    return run


def slices_rule(pinned, ntasks, max_n):
    """kernels.hip msm_tblw_slices for the two-window waves, restated from its comment: the option pins it; otherwise several waves
    per window of a task only while the GPU would stand almost empty (16 waves per task against 1024 SIMDs), and only while a slice
    keeps at least 256 points"""
    if pinned:
        return pinned
    waves = 16 * ntasks
    s = 4 if 4 * waves <= 1024 else 2 if 2 * waves <= 1024 else 1
    while s > 1 and max_n // s < 256:
        s //= 2
    return s


@pytest.mark.parametrize("pinned", [0, 1, 2, 4])
@pytest.mark.parametrize("lens", LENGTH_LISTS, ids=lambda l: "x".join(map(str, l[:4])) + ("_%d" % len(l)))
def test_offsets_are_disjoint_in_order_and_add_up(emul, lens, pinned):
    pl = emul("msm", pinned, *lens)
    count, points, max_n = len(lens), sum(lens), max(lens, default=0)
    assert pl["refused"] == 0 and pl["count"] == count and pl["points"] == points and pl["max_n"] == max_n
    slices = pl["slices"]
    assert slices == slices_rule(pinned, count, max_n)
    # scratch sizes = the sum of what the tasks need: 2 table-form entries (P, -phi(P)) and 9 digit words per point, 32 bucket sets per
    # task and slice (16 windows x lower / upper half), as many partial sums; the tail adds 2 * slices partial sums per weight
    assert pl["conv_entries"] == sum(2 * n for n in lens) and pl["digit_words"] == sum(9 * n for n in lens)
    assert pl["sets"] == count * 32 * slices and pl["tail_dup"] == 2 * slices
    assert len(pl["task"]) == count
    conv_end = dig_end = part_end = off = 0
    for i, (n, row) in enumerate(zip(lens, pl["task"])):
        idx, conv_off, conv_first, dig_first, part_first, slot_lo, slot_hi = row
        assert idx == i and conv_off == off                        # the task's points in the uploaded bases / scalars: task after task
        assert conv_first == conv_end and dig_first == dig_end and part_first == part_end      # in order, no gap, no overlap
        assert conv_first == 2 * conv_off and dig_first == 9 * conv_off                         # ... and where k_to_table_endo puts them
        assert slot_lo == part_first and slot_hi == part_first + 32 * slices - 1                # part[(16 i + w) * 2 slices + d]
        off += n
        conv_end += 2 * n
        dig_end += 9 * n
        part_end += 32 * slices
    assert conv_end == pl["conv_entries"] and dig_end == pl["digit_words"] and part_end == pl["sets"]


def test_the_lists_reach_every_value_of_the_rule():
    assert {slices_rule(0, len(l), max(l, default=0)) for l in LENGTH_LISTS} == {1, 2, 4}
    assert slices_rule(0, 4, 1030) == 4 and slices_rule(0, 4, 1023) == 2 and slices_rule(0, 1, 511) == 1 and slices_rule(0, 1, 512) == 2
    assert slices_rule(0, 16, 1024) == 4 and slices_rule(0, 17, 1024) == 2 and slices_rule(0, 32, 4096) == 2 and slices_rule(0, 33, 4096) == 1


def test_limits_are_checked_before_the_lengths_are_read(emul):
    assert emul("refuse", (1 << 16) + 1)["refused"] == 1           # lens is NULL in this call: a read would be the sanitizer's
    assert emul("refuse", 0)["refused"] == 0
    ok = emul("points", 1 << 10, 1 << 14)                          # 2^24 points in 2^14 tasks: the most a call takes
    assert ok["refused"] == 0 and ok["points"] == 1 << 24
    assert emul("points", (1 << 10) + 1, 1 << 14)["refused"] == 1
    assert emul("points", 0xffffffff, 3)["refused"] == 1           # no 32-bit wrap on the way to the limit
    assert emul("points", 1, 1 << 16)["refused"] == 0 and emul("points", 1, (1 << 16) + 1)["refused"] == 1


@pytest.mark.parametrize("families,half", [(1, 1), (2, 128), (3, 128), (3, 341), (2, 512), (3, 342), (1, 1025), (3, 512)])
def test_fold_form_follows_the_option(emul, families, half):
    total = families * half
    for quad_max in (0, 1, 384, 1024, 1 << 20):
        for plain in (0, 1):
            r = emul("fold", families, half, quad_max, plain)
            want_quad = not plain and quad_max > 0 and total <= quad_max
            assert r["fits"] == 1 and r["quad_max"] == (quad_max if want_quad else 0), (families, half, quad_max, plain)


def test_fold_limit(emul):
    assert emul("fold", 1, 1 << 24, 1024, 0)["fits"] == 1 and emul("fold", 1, (1 << 24) + 1, 1024, 0)["fits"] == 0
    assert emul("fold", 3, (1 << 24) // 3, 1024, 0)["fits"] == 1 and emul("fold", 3, (1 << 24) // 3 + 1, 1024, 0)["fits"] == 0
    assert emul("fold", 1 << 40, 1 << 40, 1024, 0)["fits"] == 0    # no 64-bit wrap in the product
    assert emul("fold", 0, 1 << 60, 1024, 0)["fits"] == 1          # nothing to do
