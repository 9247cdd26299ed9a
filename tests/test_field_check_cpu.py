"""The host twin of tests/device/field_check.hip: the field and point headers of curdleproofs_amd/csrc (mont32.hpp, fp28.hpp,
g1_28.hpp) compiled by g++ as plain C++, every operation on raw limbs over every operand set of tests/f28_vectors.py, against Python
integers (products: the exact Montgomery relation; mont32: the canonical residue; linear operations: the exact integer with
normalised limbs; point formulas: the oracle, as points).  This pins the harness that tests/test_gpu_field.py runs on the device
(file format, operation table, row counts) without a GPU, and checks f28_product_is_zero and the conversions on the host."""
import struct
import subprocess

import pytest

from tests import f28_vectors as fv
from tests import field_check_lib as fc


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return fc.build_host_twin(tmp_path_factory.mktemp("field_check"))


def test_operation_table(twin):
    """the program's own table is the one the tests drive: same names, same row widths, and every operation belongs to a group"""
    assert fc.list_operations(twin) == fc.TABLE
    assert {fc.group_of(n) for n in fc.TABLE} == set(fc.GROUPS)


def test_kernel_instantiations_are_in_the_table():
    """what the kernels instantiate (grep of curdleproofs_amd/csrc): xyzz28_add_mixed_t<false> as xyzz28_add_mixed / t_acc_add_mixed
    and xyzz28_add_mixed_t<true, F28_KARA, F28_REDC_KARA> as t_acc_add_mixed_inl (no kernel passes another choice), which use
    f28_mul<true, true>, f28_sqr<true> and f28_mul_body / f28_sqr_body / f28_mulsub_body<true, true>; every other formula calls the
    defaults f28_mul<>, f28_sqr<>, f28_mulsub_body<>"""
    for name in ("xyzz28_add_mixed", "xyzz28_add_mixed_inl", "xyzz28_add_mixed_t/1,1,1", "f28_mul/2", "f28_mul/-1", "f28_sqr/2", "f28_sqr/-1",
                 "f28_mul_body/2", "f28_sqr_body/2", "f28_mulsub_body/2", "f28_mulsub_body/-1"):
        assert name in fc.TABLE


@pytest.mark.parametrize("group", fc.GROUPS)
def test_every_operation_against_integers(twin, orc, tmp_path, group):
    records = fc.group_records(group, orc)
    assert {n for n, _ in records} == {n for n in fc.TABLE if fc.group_of(n) == group}      # no operation without rows
    total = sum(len(rows) for _, rows in records)
    assert all(rows for _, rows in records)
    got = fc.run(twin, records, tmp_path, group, timeout=600)
    assert fc.check_integers(records, got, fc.PointChecks(orc), who="host twin") == total
    if group == "f28_products":       # every body sums the same integer columns: identical limbs
        by = dict(got)
        for op, bodies in (("f28_mul_body", fc.BODIES3), ("f28_mul", fc.BODIES3), ("f28_mulsub_body", fc.BODIES3), ("f28_sqr_body", fc.SQR_BODIES),
                           ("f28_sqr", fc.SQR_BODIES)):
            for b in bodies[1:]:
                assert (by[op + "/" + b] == by[op + "/0"]).all(), (op, b)
        assert (by["f28_mul/0"] == by["f28_mul_body/0"]).all() and (by["f28_sqr/0"] == by["f28_sqr_body/0"]).all()
    if group == "points":             # the mixed addition with any choice of bodies: identical limbs (the inlined form ends in the
        by = dict(got)                # shared reduction of Y3, another representative than the two products of the called form)
        for m in ("xyzz28_add_mixed_t/1,1,1", "xyzz28_add_mixed_t/1,1,0", "xyzz28_add_mixed_t/1,0,0"):
            assert (by[m] == by["xyzz28_add_mixed_inl"]).all(), m
        assert (by["xyzz28_add_mixed_t/0,0,0"] == by["xyzz28_add_mixed"]).all()


def test_mont32_vectors_reach_the_carry_word():
    """the named pairs of the mont32 set do what their names say (tests/f28_vectors.py: mont_columns): the 64-bit accumulator wraps
    into c2 in the first and in the last column that operands below the modulus can reach, in many, and in none; digits all 0 / all
    0xffffffff"""
    for f, (singles, pairs, named) in fc.mont_vectors().items():
        p, n = fc.FIELDS[f]
        assert all(0 <= a < p and 0 <= b < p for a, b in pairs) and all(0 <= a < p for a in singles)
        assert all(pair in pairs for pair in named.values())
        cols = {k: fv.mont_columns(a, b, p, n) for k, (a, b) in named.items()}
        first = [k for k in named if k.startswith("c2_first_column_")][0]
        last = [k for k in named if k.startswith("c2_last_column_")][0]
        kf, kl = int(first.rsplit("_", 1)[1]), int(last.rsplit("_", 1)[1])
        assert kf == (0 if f == "fp" else 1) and cols[first][0][kf] >= 1 and not any(cols[first][0][:kf])
        assert kl >= n and cols[last][0][kl] >= 1 and not any(cols[last][0][kl + 1:])
        assert not any(cols["c2_no_column"][0]) and min(named["c2_no_column"]) > 1
        assert sum(1 for w in cols["c2_most_columns"][0] if w) >= n
        assert max(cols["c2_most_columns"][0]) >= 4                 # c2 counts, it is not a flag
        for j in range(3):
            assert set(cols["digits_zero_%d" % j][1]) == {0} and set(cols["digits_ones_%d" % j][1]) == {0xffffffff}
            assert cols["digits_low_ones_%d" % j][1] == [0xffffffff] * (n // 2) + [0] * (n // 2)
            assert cols["digits_high_ones_%d" % j][1] == [0] * (n // 2) + [0xffffffff] * (n // 2)


def test_product_is_zero_named_values(twin, tmp_path):
    """0 and p are zero; 1, p - 1, p + 1, -1 (top limb negative) are not; 2 p lies outside the range of a product and is not accepted"""
    P = fv.P
    vals = [0, P, 1, P - 1, P + 1, -1, 2 * P]
    records = [("f28_product_is_zero", [fv.limbs(v) for v in vals])]
    got = fc.run(twin, records, tmp_path, "piz")
    assert got[0][1][:, 0].tolist() == [1, 1, 0, 0, 0, 0, 0]
    assert fv.limbs(-1)[13] == -1
    assert fc.check_integers(records, got) == len(vals)


def test_the_checks_notice_a_wrong_result(twin, tmp_path):
    """the integer checks are not vacuous: one flipped bit in a result fails, naming the operation, the row and the operands"""
    records = [("f28_mul_body/2", [fv.limbs(3) + fv.limbs(5)] * 3), ("fp_mul", [fv.words32(7, 12) + fv.words32(9, 12)] * 2)]
    got = fc.run(twin, records, tmp_path, "ok")
    assert fc.check_integers(records, got) == 5
    for rec, row in ((0, 2), (1, 1)):
        bad = [(n, a.copy()) for n, a in got]
        bad[rec][1][row, 4] ^= 1
        with pytest.raises(AssertionError, match=r"%s row %d: .*\n  in  \[0x" % (records[rec][0], row)):
            fc.check_integers(records, bad)
        with pytest.raises(AssertionError, match=r"%s row %d: device and host twin differ" % (records[rec][0], row)):
            fc.assert_same(records, bad, got)
    assert fc.assert_same(records, got, got) == 5


def test_bad_records_are_refused(twin, tmp_path):
    """an unknown operation, a wrong row width and a truncated record end the program with a non-zero exit code"""
    row = struct.pack("<14I", *([1] * 14))
    for tag, blob in (("unknown", struct.pack("<48sIIQ", b"f28_nothing", 14, 0, 1) + row),
                      ("width", struct.pack("<48sIIQ", b"f28_neg", 13, 0, 1) + row),
                      ("short", struct.pack("<48sIIQ", b"f28_neg", 14, 0, 2) + row),
                      ("tail", struct.pack("<48sIIQ", b"f28_neg", 14, 0, 1) + row + b"\0\0\0")):
        inp = tmp_path / (tag + ".in")
        inp.write_bytes(blob)
        r = subprocess.run([twin, str(inp), str(tmp_path / (tag + ".out"))], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "field_check:" in r.stderr, tag
