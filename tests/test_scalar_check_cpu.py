"""The host twin of tests/device/scalar_check.hip: the scalar-side headers of curdleproofs_amd/csrc (glv.hpp, recode.hpp, gen_table.hpp,
tracker_ladder.hpp, modinv30.hpp and the inversions, powers and compares of mont32.hpp) compiled by g++ as plain C++, every function
over the rows of tests/scalar_cases.py, against Python integers and the contract each header documents (tests/scalar_check_lib.py).
This pins the harness that tests/test_gpu_scalar.py runs on the device (file format, operation table, row counts) without a GPU, states
what the case set covers, and runs the twin once under the undefined-behaviour and address sanitizers: the shifts, the borrow chains and
the int8_t / int16_t narrowings are what that run is for."""
import struct
import subprocess

import pytest

from tests import scalar_cases as sc
from tests import scalar_check_lib as sl
from tests.scalar_cases import P, R, Z2, H2


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return sl.build_host_twin(tmp_path_factory.mktemp("scalar_check"))


def test_operation_table(twin):
    """the program's own table is the one the tests drive: same names, same row widths, and every operation belongs to a group"""
    assert sl.list_operations(twin) == sl.TABLE
    assert {sl.group_of(n) for n in sl.TABLE} == set(sl.GROUPS)


def test_kernel_instantiations_are_in_the_table():
    """what the kernels instantiate (kernels.hip: k_msm_fix<19, 7>, <16, 16>, <16, 8>, <16, 4>, <16, 2>, <8, 16>, <8, 8>, each wave group
    wg calling fix_window_digits<CB, FIX_WPW> with w0 = wg FIX_WPW; late.hip: k_late_fix<19>, <16>, <8> on FixDigitStream<CB>)"""
    for cb, nw in ((19, 7), (16, 16), (16, 8), (16, 4), (16, 2), (8, 16), (8, 8)):
        assert "fix_window_digits/%d,%d" % (cb, nw) in sl.TABLE and sc.fix_windows(cb) % nw == 0
    for cb in (8, 16, 19):
        assert "fix_digit_stream/%d" % cb in sl.TABLE


@pytest.mark.parametrize("group", sl.GROUPS)
def test_every_operation_against_integers(twin, tmp_path, group):
    records = sl.group_records(group)
    assert {n for n, _ in records} >= {n for n in sl.TABLE if sl.group_of(n) == group}      # no operation without rows
    total = sum(len(rows) for _, rows in records)
    assert all(rows for _, rows in records)
    got = sl.run(twin, records, tmp_path, group, timeout=600)
    assert sl.check_integers(records, got, who="host twin") == total
    assert sl.check_across(records, got, who="host twin") == sl.across_count(group, records)


def test_scalar_case_set_covers_the_split():
    """each property with a row present: both values of neg_k and of neg_t and all four combinations (the fold of recode_smul_glv is
    neg_k ^ neg_t), t = 0, q = 0, the longest forms of both halves, every directed scalar.
    A half is below 2^127 - 2^119, so its non-adjacent form ends at bit 127 at the latest: bit 128 (word 4 of SmulNaf) is empty for every
    scalar below r, and the checks of recode_smul_glv, glv_table_entry and tracker_ladder_step assert that for every row.  What the set
    must reach is the top: a digit at bit 127 in either half."""
    s = sl.case_sets()["scalars"]
    assert all(v in s for v in sc.EDGE_SCALARS.values()) and len(s) >= 4000
    for name in ("0", "1", "2", "r-1", "r-2", "(r-1)/2", "(r+1)/2", "z2", "z2-1", "z2+1", "z2/2", "z2/2-1", "z2/2+1", "r-z2", "(r-1)/2-z2/2", "2^127",
                 "2^128-1", "2^254", "2^255 mod r", "(2^127-1) z2", "qmax z2"):
        assert name in sc.EDGE_SCALARS
    splits = [sc.py_split(k) for k in s]
    for k, (t, q, nk, nt) in zip(s, splits):
        assert ((-1) ** nk * ((-1) ** nt * t + q * Z2)) % R == k
    assert {(nk, nt) for _, _, nk, nt in splits} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(t == 0 and k for k, (t, _, _, _) in zip(s, splits)) and any(q == 0 and k for k, (_, q, _, _) in zip(s, splits))
    assert any(q == sc.Q_MAX for _, q, _, _ in splits) and any(t == H2 for t, _, _, _ in splits)
    assert sc.py_split((R - 1) // 2)[2] == 0 and sc.py_split((R + 1) // 2)[2] == 1                 # the sign of k turns between them
    assert sc.py_split(H2 - 1)[3] == 0 and sc.py_split(H2)[3] == 1                                   # and the sign of t here (z^2 is even)
    assert max(len(sc.naf(t)) for t, _, _, _ in splits) == 128 and max(len(sc.naf(q)) for _, q, _, _ in splits) == 128
    assert len(sc.naf(sc.HALF_BOUND - 1)) <= 128
    for b in range(255):
        assert 1 << b in s and (1 << b) - 1 in s
    ladder = sl.ladder_scalars()
    assert all(v in ladder for v in sc.EDGE_SCALARS.values()) and len(ladder) == 1500


def test_naf_case_set_reaches_the_257th_digit():
    """the plain form of k_smul recodes all eight words: rows whose form has a digit at bit 256, rows with a digit at bit 128, and the
    alternating patterns with the longest carry runs"""
    rows = sl.case_sets()["naf"]
    assert any(len(sc.naf(v)) == 257 for v in rows) and any(len(sc.naf(v)) > 128 and sc.naf(v)[128] for v in rows)
    for pat in ("55", "aa", "33"):
        assert int(pat * 32, 16) in rows
    assert all(0 <= v < (1 << 256) for v in rows) and len(rows) >= 4000


@pytest.mark.parametrize("cb", sc.FIX_CB)
def test_scalar_case_set_carries_out_of_every_window(cb):
    """for every window but the top one, a row whose chunk reaches the carry threshold 2^(cb-1) and one whose chunk is one below it;
    no scalar below r can carry out of the top window"""
    s = sl.case_sets()["scalars"]
    w, half, mask = sc.fix_windows(cb), 1 << (cb - 1), (1 << cb) - 1
    at, below, carried = set(), set(), set()
    for k in s:
        carry = 0
        for j in range(w):
            x = ((k >> (cb * j)) & mask) + carry
            if x == half and not carry:
                at.add(j)
            if x == half - 1 and not carry:
                below.add(j)
            carry = 1 if x >= half else 0
            if carry:
                carried.add(j)
        assert carry == 0, hex(k)
    top = {j for j in range(w) if (half << (cb * j)) < R}
    assert at >= top and below >= top and carried >= set(range(w - 1))


def test_biased_bytes_bound_is_the_documented_one(twin, tmp_path):
    """Regression: glv.hpp used to promise the 16 signed bytes for every value below 2^127; 2^127 - 1 (and everything from 0x7f7f...80
    on) wraps the biased sum out of 128 bits.  The documented bound is now 0x7f7f...7f, the largest value 16 digits in [-128, 127] have:
    it and the largest halves glv_split returns reconstruct exactly, and the row that showed it stays in the half-size case set for the
    nibble recoding, whose bound 2^127 holds."""
    assert sc.BIASED_MAX == sum(127 << (8 * w) for w in range(16)) and sc.H2 + 1 < sc.BIASED_MAX and sc.Q_MAX < sc.BIASED_MAX
    records = [("glv_biased_bytes", [sl.words(v, 4) for v in (sc.BIASED_MAX, sc.BIASED_MAX - 1, sc.H2 + 1, sc.Q_MAX)])]
    got = sl.run(twin, records, tmp_path, "biased")
    assert sl.check_integers(records, got) == 4 and got[0][1][0].tolist() == [0xffffffff] * 4
    assert (1 << 127) - 1 in sl.case_sets()["halves"] and (1 << 127) - 1 > sc.BIASED_MAX


def test_half_case_set():
    h = sl.case_sets()["halves"]
    for v in (int("8" * 31, 16), int("9" * 31, 16), int("80" * 15, 16), int("7f" * 16, 16), (1 << 127) - 1, 0):
        assert v in h
    assert len(h) >= 4000


@pytest.mark.parametrize("p,bits,high,measured", [(P, 381, sc.HIGH_COUNT_P, 28), (R, 255, sc.HIGH_COUNT_R, 19)], ids=["p", "r"])
def test_inversion_inputs_and_batch_counts(p, bits, high, measured):
    """The batches of 30 division steps every inversion input takes, counted by the integer restatement (scalar_cases.batch_count),
    stay below MAX_BATCHES of modinv30.hpp: 40 for p, 28 for r.  Measured maxima over the set, on the CPU: 28 batches for p (the
    hard-coded results of the seeded search; random 381-bit values take 18 to 26) and 19 for r (random 255-bit values take 12 to 18).
    The search that found the hard-coded inputs takes 10 s at its full size; here it runs at a twentieth of it, to keep it alive, and must
    find nothing above the measured maximum.  batch_count steps over runs of zeros at once; on the directed inputs and the high-count ones it
    must count what single batches of scalar_check_lib.divsteps30, the restated batch of modinv30.hpp, count."""
    inputs = sl.case_sets()["inv_p" if p == P else "inv_r"]
    for v in (0, 1, p - 1, (p - 1) // 2, (p + 1) // 2, 1 << 30, (1 << 30) - 1, 0x3fffffff << 30, (1 << 60) + 1):
        assert v in inputs
    for b in range(bits):
        assert 1 << b in inputs and (1 << (b + 1)) - 1 in inputs or (1 << (b + 1)) - 1 >= p
    assert all(v in inputs for v in high) and 1200 <= len(inputs) <= 1600
    counts = [sc.batch_count(v, p) for v in inputs if v]
    assert max(counts) == measured < sl.MAX_BATCHES[p]
    assert all(sc.batch_count(v, p) == measured for v in high)
    for v in [x for x in inputs[:60] if x] + list(high):
        eta, f, g, n = -1, p, v, 0
        while True:
            eta, _, f, g = sl.divsteps30(eta, f, g)
            n += 1
            if g == 0:
                break
        assert n == sc.batch_count(v, p) and abs(f) == 1, hex(v)
    small = sc.batch_search(p, bits, 1000, 256, keep=4)
    assert max(sc.batch_count(v, p) for v in small) <= measured


def test_divsteps_rows_cover_eta_and_the_low_words():
    rows = sl.case_sets()["divsteps"]
    assert all(f & 1 and 0 <= f < (1 << 30) and 0 <= g < (1 << 30) for _, f, g in rows)
    etas = {eta for eta, _, _ in rows}
    assert etas >= set(range(-800, 801))          # beyond +-(2 x 383): what 40 batches on 381-bit inputs can reach
    for want in ((lambda f, g: g == 0), (lambda f, g: g & 1), (lambda f, g: g and not g & 1), (lambda f, g: f == 1), (lambda f, g: f == (1 << 30) - 1)):
        assert any(want(f, g) for _, f, g in rows)
    # the restated batch agrees with single division steps on the full integers: the reference of the matrix check
    for eta, f, g in rows[:200]:
        e1, (u, v, q, r), f1, g1 = sl.divsteps30(eta, f, g)
        assert u * f + v * g == f1 << 30 and q * f + r * g == g1 << 30 and f1 & 1


def test_twin_under_sanitizers(tmp_path):
    """the twin built with -fsanitize=undefined,address (no recovery) as a stand-alone program, over the directed part of every group: a
    shift by the word size, a signed overflow or a narrowing out of range in the headers ends it with a report"""
    exe = sl.build_host_twin(tmp_path, extra=["-O1", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"], name="scalar_check_san")
    for group in sl.GROUPS:
        records = [(n, rows[:120] + rows[-20:]) for n, rows in sl.group_records(group)]
        got = sl.run(exe, records, tmp_path, "san_" + group, timeout=600)
        assert sl.check_integers(records, got, who="sanitized twin") == sum(len(r) for _, r in records)


def test_the_checks_notice_a_wrong_result(twin, tmp_path):
    """the integer checks are not vacuous: one flipped bit in a result fails, naming the operation, the row and the input words"""
    k = sl.words(sc.EDGE_SCALARS["r - z2/2 - 1"], 8)
    records = [("glv_split", [k] * 2), ("recode_smul_glv", [k] * 3), ("fix_digit_stream/19", [k] * 2), ("fr_inv_divsteps", [k] * 2), ("gen_pick", [k] * 2),
               ("recode_naf", [k] * 2), ("glv_table_entry", [k] * 2)]
    got = sl.run(twin, records, tmp_path, "ok")
    total = sum(len(r) for _, r in records)
    assert sl.check_integers(records, got) == total
    for rec in range(len(records)):
        for word in (0, 1):
            bad = [(n, a.copy()) for n, a in got]
            bad[rec][1][1, word] ^= 1
            with pytest.raises(AssertionError, match=r"%s row 1: .*\n  in  \[0x" % records[rec][0]):
                sl.check_integers(records, bad)
            with pytest.raises(AssertionError, match=r"%s row 1: device and host twin differ" % records[rec][0]):
                sl.assert_same(records, bad, got)
    assert sl.assert_same(records, got, got) == total


def test_bad_records_are_refused(twin, tmp_path):
    """an unknown operation, a wrong row width and a truncated record end the program with a non-zero exit code"""
    row = struct.pack("<8I", *([1] * 8))
    for tag, blob in (("unknown", struct.pack("<48sIIQ", b"glv_nothing", 8, 0, 1) + row),
                      ("width", struct.pack("<48sIIQ", b"glv_split", 7, 0, 1) + row),
                      ("short", struct.pack("<48sIIQ", b"glv_split", 8, 0, 2) + row),
                      ("tail", struct.pack("<48sIIQ", b"glv_split", 8, 0, 1) + row + b"\0\0\0")):
        inp = tmp_path / (tag + ".in")
        inp.write_bytes(blob)
        r = subprocess.run([twin, str(inp), str(tmp_path / (tag + ".out"))], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "scalar_check:" in r.stderr, tag
