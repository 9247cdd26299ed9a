"""CPU side of the quad check (tests/device/quad_check.hip, run on the GPU by tests/test_gpu_quad.py): the operation table equals the
cross-compiled program's, the row generators of tests/quad_check_lib.py reach what they claim (asserted from the integers alone), the
program refuses bad records before it touches a device, and the checker is pinned without device code: the results of the ONE-LANE
formulas (xyzz28_add, xyzz28_dbl, jac28_dbl, the field products and inversion of the field_check host twin, chained in Python for the
chain and ladder rows), replicated over four lanes with the expected codes attached, are accepted row for row, and a flipped bit in one
lane, a wrong code, a coordinate moved by 8 p, the negated point and an inverse multiplied by 2 are each rejected."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import field_check_lib as fc
from tests import quad_check_lib as ql
from tests.f28_vectors import P, R392, limbs, value, words32
from tests.field_check_lib import _xyzz_of, _jac_of, _s32, _split, _words
from tests.quad_check_lib import OK, TAKE_Q, TAKE_P, DOUBLE_P, IDENTITY, COMBOS, WAVE


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return fc.build_host_twin(tmp_path_factory.mktemp("field_check"))


@pytest.fixture(scope="module")
def program():
    """the gfx950 build of the program; here only its host side runs (--list and the records it refuses)"""
    from curdleproofs_amd import build as b
    assert ("quad_check", "standalone") in [(n, k) for n, (_, k) in b.CHECKS.items()]
    exe = b.build_check("quad_check")
    assert exe == b.check_path("quad_check") and os.path.dirname(exe) == os.path.dirname(b.LIB)
    with open(exe, "rb") as f:
        assert b"gfx950" in f.read()
    return exe


@pytest.fixture(scope="module")
def qv(orc):
    return ql.QuadVectors(orc)


def test_operation_table(program):
    assert ql.list_operations(program) == ql.TABLE
    assert len(ql.TABLE) == 11 and set(ql.PARAMETERS) < set(ql.TABLE) and set(ql.INVERSIONS) < set(ql.TABLE)
    from curdleproofs_amd import build as b
    assert len((b.FIELDCHECK, b.TRANSCRIPTCHECK, b.SCALARCHECK, b.RNGCHECK, b.RNGG1CHECK, b.MSMCHECK)) == 6      # the legacy names still unpack
    assert b.MSMCHECK == b.check_path("msm_check")


def test_bad_records_are_refused(program, tmp_path):
    """exit 3 and an empty output file, judged from the table, the widths and the parameter word before any device call"""
    one = limbs(R392 % P)
    xyzz = one * 4
    rec = lambda name, width, rows: struct.pack("<48sIIQ", name.encode(), width, 0, len(rows)) + np.array(rows, dtype="<u4").tobytes()
    cases = [("unknown", rec("xyzz28_add_quad", 112, [xyzz * 2])),
             ("width", rec("xyzz28_dbl_quad", 57, [xyzz + [0]])),
             ("width_core", rec("xyzz28_add_quad_core", 113, [xyzz * 2 + [0]])),
             ("inverse63", rec("t_block_batch_inverse/64", 14, [one] * 63)),
             ("inverse64of256", rec("t_block_batch_inverse/256", 14, [one] * 64)),
             ("std_inverse65", rec("block_batch_inverse/64", 12, [words32(1, 12)] * 65)),
             ("std_inverse255", rec("block_batch_inverse/256", 12, [words32(1, 12)] * 255)),
             ("count0", rec("jac28_dbl_quad/chain", 43, [one * 3 + [1], one * 3 + [0]])),
             ("count129", rec("jac28_dbl_quad/chain", 43, [one * 3 + [129]])),
             ("pattern17bits", rec("xyzz28_quad_ladder", 113, [xyzz * 2 + [0x10000]])),
             ("flag2", rec("xyzz28_add_quad_mem", 113, [xyzz * 2 + [2]])),
             ("short", rec("xyzz28_dbl_quad", 56, [xyzz])[:-4]),
             ("tail", rec("jac28_dbl_quad/chain", 43, [one * 3 + [300]]) + b"\0")]
    for name, (lo, hi) in ql.PARAMETERS.items():      # the bounds the cases step over are the table's
        assert ql.TABLE[name][0] in (43, 113)
    assert ql.PARAMETERS["jac28_dbl_quad/chain"] == (1, 128)
    for tag, blob in cases:
        inp, outp = tmp_path / (tag + ".in"), tmp_path / (tag + ".out")
        inp.write_bytes(blob)
        r = subprocess.run([program, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 3 and "quad_check:" in r.stderr, (tag, r.returncode, r.stderr)
        assert outp.read_bytes() == b"", tag


# ---------------------------------------------------------------- the rows reach what they claim

def _combo(row, wide=False):
    """per coordinate of an XYZZ operand: "lo" / "hi" if it is the first / last representative of its documented range (wide: X and Y
    in the range of a Jacobian point), "out" if it lies outside, else None"""
    out = []
    xy = ((-1540, 1540), (-1540, 1540)) if wide else ((-630, 630), (-270, 270))
    for c, (lo, hi) in zip(_split(row, 14), xy + ((-81, 181), (-81, 181))):
        v = value(c)
        inside = lo * P < 100 * v < hi * P
        out.append("out" if not inside else "lo" if 100 * (v - P) <= lo * P else "hi" if 100 * (v + P) >= hi * P else None)
    return tuple(out)


def test_addition_rows_hold_every_outcome_and_the_extreme_representatives(qv):
    core, mem = qv.add_rows(), qv.mem_rows()
    for rows in (core, mem):
        assert {ql.add_row_code(r) for r in rows} == {OK, TAKE_Q, TAKE_P, DOUBLE_P, IDENTITY}
    # P + P and P - P on the same and on different ZZ; the identity on either and on both sides
    same = {(ql.add_row_code(r), r[28:42] == r[84:98]) for r in core if ql.add_row_code(r) in (DOUBLE_P, IDENTITY)}
    assert same == {(DOUBLE_P, True), (DOUBLE_P, False), (IDENTITY, True), (IDENTITY, False)}
    assert any(not any(r[28:42]) and not any(r[84:98]) for r in core)
    # same-slot rows: generic points and the identity
    slot = [r for r in mem if r[112]]
    assert {ql.add_row_code(r) for r in slot} == {DOUBLE_P, TAKE_Q} and len(slot) >= 50
    # all-low, all-high and alternating, on both operands, for at least eight accumulators
    pairs, points = set(), set()
    for r in core:
        if not any(r[28:42]) or not any(r[84:98]):
            continue
        cp, cq = _combo(r[:56]), _combo(r[56:])
        if cp in COMBOS and cq in COMBOS:
            pairs.add((cp, cq))
            points.add(_xyzz_of(r[:56]))
    assert pairs == {(a, b) for a in COMBOS for b in COMBOS} and len(points) >= 8
    # operands as xyzz28_from_jac hands them on: X and Y at the ends of the Jacobian range, every outcome but the identity operands
    wide = [r for r in core if "out" in _combo(r[:56]) and _combo(r[:56], True) in COMBOS and _combo(r[56:], True) in COMBOS]
    assert {ql.add_row_code(r) for r in wide} == {OK, DOUBLE_P, IDENTITY} and {_combo(r[:56], True) for r in wide} == set(COMBOS)
    assert any(abs(value(r[:14])) > 14 * P and abs(value(r[14:28])) > 14 * P for r in wide)
    assert all("out" not in _combo(r[:56], True) + _combo(r[56:112], True) for r in core + mem if any(r[28:42]) and any(r[84:98]))
    # the extreme rows sit at the first and last representative: one p further leaves the range
    acc = qv.accs[3][0]
    for c in COMBOS:
        assert _combo(qv.xyzz(acc, 7, c)) == c
        x, y, z = (value(v) for v in _split(qv.jac(acc, 7, c[:3]), 14))
        for v, bound, pick in ((x, 1540, c[0]), (y, 1540, c[1]), (z, 360, c[2])):
            assert -bound * P < 100 * v < bound * P
            assert 100 * (v - P) <= -bound * P if pick == "lo" else 100 * (v + P) >= bound * P


def test_row_order_mixed_waves_and_whole_waves(qv):
    records = qv.add_records()
    assert [n for n, _ in records] == ["xyzz28_add_quad_core"] * 2 + ["xyzz28_add_quad_mem"] * 2
    for (_, mixed), (_, whole), src in ((records[0], records[1], qv.add_rows()), (records[2], records[3], qv.mem_rows())):
        assert len(mixed) % WAVE == 0 and len(whole) % WAVE == 0 and len(mixed) >= 16 * WAVE
        for w in range(0, len(mixed), WAVE):
            assert {ql.add_row_code(r) for r in mixed[w:w + WAVE]} == {OK, TAKE_Q, TAKE_P, DOUBLE_P, IDENTITY}
        waves = [{ql.add_row_code(r) for r in whole[w:w + WAVE]} for w in range(0, len(whole), WAVE)]
        assert all(len(s) == 1 for s in waves) and set().union(*waves) == {OK, TAKE_Q, TAKE_P, DOUBLE_P, IDENTITY}
        assert {tuple(r) for r in whole} == {tuple(r) for r in src} and 200 <= len(src) <= 1000      # every row is in the whole-wave record


def test_doubling_chain_and_ladder_rows(qv):
    xr, jr = qv.xyzz_rows(), qv.jac_rows()
    assert sum(1 for r in xr if not any(r[28:42])) == 1 + WAVE and sum(1 for r in jr if not any(r[28:])) == 1 + WAVE
    assert {_combo(r) for r in xr if any(r[28:42])} >= set(COMBOS)
    assert {_combo(r, True) for r in xr if any(r[28:42]) and "out" in _combo(r)} == set(COMBOS)      # and in the Jacobian range of X, Y
    one = limbs(R392 % P)
    assert any(r[28:42] == one for r in xr) and any(r[28:42] != one and _combo(r) not in COMBOS for r in xr)      # scale 1 and a random scale
    (_, chain), = qv.chain_records()
    assert {r[42] for r in chain} == set(ql.COUNTS) and ql.COUNTS == (1, 2, 8, 56, 120)
    for n in ql.COUNTS:
        rows = [r for r in chain if r[42] == n]
        assert any(r[28:42] == one for r in rows) and any(not any(r[28:42]) for r in rows)                          # normalised, the identity
        assert any(abs(value(r[:14])) > 14 * P and abs(value(r[28:42])) > 2 * P for r in rows)                       # extreme
    ladder = qv.ladder_rows()
    pats = [r[112] for r in ladder]
    assert set(ql.PATTERNS) <= set(pats) and len(set(pats)) >= 8
    traces = [(_xyzz_of(r[:56]), _xyzz_of(r[56:112]), r[112], ql.ladder_trace(_xyzz_of(r[:56]), _xyzz_of(r[56:112]), r[112])[0]) for r in ladder]
    from_identity = [t for t in traces if t[0] is None]
    assert {t[2] for t in from_identity} >= set(ql.PATTERNS) and all(t[3][:1] in ([], [TAKE_Q]) for t in from_identity)
    from_q = [t for t in traces if t[0] is not None and t[0] == t[1]]
    assert {t[2] for t in from_q} >= set(ql.PATTERNS) and all(t[3][0] == OK for t in from_q if t[2] >> 15)              # 2 P + P
    from_neg = [t for t in traces if t[0] is not None and t[0] == ql._neg(t[1])]
    assert {t[2] >> 15 for t in from_neg} == {0, 1}
    assert any(IDENTITY in t[3][:-1] for t in traces) and any(DOUBLE_P in t[3] for t in traces)                        # met in mid-chain
    assert any(t[3][:1] == [IDENTITY] for t in traces) and any(t[2] >> 14 == 1 and t[3][:1] == [IDENTITY] for t in traces)
    assert any(t[3] and t[3][0] == IDENTITY and TAKE_Q in t[3] for t in traces)                                         # and the chain goes on


def test_inversion_blocks(qv):
    for name, n in ql.INVERSIONS.items():
        blocks = dict(qv.inverse_blocks(name))
        assert all(len(rows) == n for rows in blocks.values())
        zeros = {k: [i for i, r in enumerate(rows) if not any(r)] for k, rows in blocks.items()}
        assert zeros["distinct"] == [] and zeros["zero at lane 0"] == [0] and zeros["zero at lane %d" % (n - 1)] == [n - 1]
        assert zeros["zero at every odd lane"] == list(range(1, n, 2)) and zeros["all zero"] == list(range(n))
        for z in (0, 37, n - 1):
            assert zeros["all zero but lane %d" % z] == [i for i in range(n) if i != z]
        assert len({tuple(r) for r in blocks["distinct"]}) == n and len({tuple(r) for r in blocks["equal values"]}) == 1
        assert ("a wave of zeros" in blocks) == (n == 256)
        if n == 256:
            assert zeros["a wave of zeros"] == list(range(64, 128))
        val = (lambda r: value(r)) if name.startswith("t_") else _words
        unit = R392 if name.startswith("t_") else fc.R384
        assert all(val(r) == unit % P for r in blocks["all ones"])
        pairs = blocks["a value next to its inverse"]
        assert all((val(pairs[i]) * val(pairs[i + 1]) - unit * unit) % P == 0 for i in range(0, n, 2))
        for rows in blocks.values():      # the accepted operand range, and nothing that is 0 mod p but the exact zero
            for r in rows:
                assert not any(r) or val(r) % P
                assert -360 * P <= 100 * val(r) <= 360 * P if name.startswith("t_") else 0 <= val(r) < P
        if name.startswith("t_"):
            vals = [value(r) for r in blocks["distinct"]]
            assert min(vals) < -P and max(vals) > 2 * P          # a Jacobian Z of either sign beyond the product range


# ---------------------------------------------------------------- the checker, pinned on the one-lane formulas

def _twin(twin, tmp, name, rows):
    """one operation of the field_check host twin over rows of words (signed limbs or the u32 words of an earlier result)"""
    if not len(rows):
        return np.zeros((0, fc.TABLE[name][1]), dtype=np.uint32)
    return fc.run(twin, [(name, [list(r) for r in rows])], tmp, "twin")[0][1].copy()


def _u32(rows, width):
    return (np.array(rows, dtype=np.int64).reshape(len(rows), width) & 0xffffffff).astype(np.uint32)


def one_lane_outputs(twin, tmp, records):
    """what a device that agrees with the one-lane formulas would write: [(name, array)] like the program's output"""
    out = []
    for name, rows in records:
        a = _u32(rows, ql.TABLE[name][0])
        if name == "xyzz28_add_quad_core":
            codes = np.array([[ql.add_row_code(r)] for r in rows], dtype=np.uint32)
            res = np.hstack([codes, _twin(twin, tmp, "xyzz28_add", a)])
        elif name == "xyzz28_add_quad_mem":
            q = np.where(a[:, 112:113] != 0, a[:, :56], a[:, 56:112])
            res = _twin(twin, tmp, "xyzz28_add", np.hstack([a[:, :56], q]))
        elif name == "xyzz28_dbl_quad":
            res = _twin(twin, tmp, "xyzz28_dbl", a)
        elif name == "jac28_dbl_quad":
            res = _twin(twin, tmp, "jac28_dbl", a)
        elif name == "jac28_dbl_quad/chain":
            res = a[:, :42].copy()
            for s in range(int(a[:, 42].max())):
                live = np.nonzero(a[:, 42] > s)[0]
                res[live] = _twin(twin, tmp, "jac28_dbl", res[live])
        elif name == "xyzz28_quad_ladder":
            res = a[:, :56].copy()
            for bit in range(15, -1, -1):
                res = _twin(twin, tmp, "xyzz28_dbl", res)
                live = np.nonzero((a[:, 112] >> bit) & 1)[0]
                res[live] = _twin(twin, tmp, "xyzz28_add", np.hstack([res[live], a[live, 56:112]]))
        elif name == "xyzz28_from_jac":      # (X, Y, Z^2, Z^3); the identity as Xyzz28::identity()
            zz = _twin(twin, tmp, "f28_sqr/-1", a[:, 28:])
            zzz = _twin(twin, tmp, "f28_mul/-1", np.hstack([zz, a[:, 28:]]))
            res = np.hstack([a[:, :28], zz, zzz])
            ident = _u32([limbs(R392 % P) * 2 + [0] * 28], 56)[0]
            for i in np.nonzero(~a[:, 28:].any(axis=1))[0]:
                res[i] = ident
        elif name.startswith("t_"):
            res = np.full_like(a, 0xa5a5a5a5)
            live = np.nonzero(a.any(axis=1))[0]
            res[live] = _twin(twin, tmp, "f28_inv_euclid", a[live])
        else:
            res = np.full_like(a, 0xa5a5a5a5)
            for i, r in enumerate(rows):
                if any(r):
                    res[i] = words32(pow(_words(r), -1, P) * fc.R384 * fc.R384 % P, 12)
        out.append((name, np.hstack([res] * 4) if name in ql.QUAD_OPS else res))
    return out


@pytest.fixture(scope="module")
def pinned(qv, twin, orc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("quad_pin")
    records = qv.add_records() + qv.dbl_records() + qv.chain_records() + qv.ladder_records() + qv.from_jac_records()
    for name in ql.INVERSIONS:
        records += qv.inverse_records(name)
    return records, one_lane_outputs(twin, tmp, records), ql.Checker(fc.PointChecks(orc))


def test_checker_accepts_the_one_lane_results(pinned, twin, tmp_path):
    records, outs, checker = pinned
    assert {n for n, _ in records} == set(ql.TABLE)                      # no operation without rows
    rows, compared = checker.check(records, outs, who="one-lane")
    assert rows == sum(len(r) for _, r in records)
    skipped = sum(1 for n, rs in records if n == "xyzz28_add_quad_core" for r in rs if ql.add_row_code(r) != OK)
    skipped += sum(1 for n, rs in records if n in ql.INVERSIONS for r in rs if not any(r))
    assert compared == rows - skipped and skipped > 0
    # the round trip of xyzz28_from_jac through the one-lane xyzz28_to_jac is the point it started from
    (name, src), (_, res) = next((r, o) for r, o in zip(records, outs) if r[0] == "xyzz28_from_jac")
    back = _twin(twin, tmp_path, "xyzz28_to_jac", res)
    assert [_jac_of(_s32(b)) for b in back.tolist()] == [_jac_of(r) for r in src]


def _edit(outs, k, fn):
    bad = [(n, a.copy()) for n, a in outs]
    fn(bad[k][1])
    return bad


def _all_lanes(a, row, lane_words, at, words):
    for lane in range(4):
        a[row, lane * lane_words + at:lane * lane_words + at + len(words)] = _u32([words], len(words))[0]


def test_checker_rejects_wrong_results(pinned):
    records, outs, checker = pinned
    rec = {}
    for k, (n, _) in enumerate(records):
        rec.setdefault(n, k)
    kc = rec["xyzz28_add_quad_core"]
    crow = next(i for i, r in enumerate(records[kc][1]) if ql.add_row_code(r) == OK and value(_s32(outs[kc][1][i, 1:15].tolist())) >= 0)

    def flip(a):
        a[crow, 2 * 57 + 5] ^= 1
    with pytest.raises(AssertionError, match=r"xyzz28_add_quad_core record %d row %d \(wave %d\) lane 2: .*differs from lane 0's\n  in  \[0x" % (kc, crow, crow // 16)):
        checker.check(records, _edit(outs, kc, flip))
    for row in (crow, next(i for i, r in enumerate(records[kc][1]) if ql.add_row_code(r) == DOUBLE_P)):      # OK -> TAKE_P, DOUBLE_P -> IDENTITY
        wrong = IDENTITY if row != crow else TAKE_P
        with pytest.raises(AssertionError, match=r"xyzz28_add_quad_core record %d row %d .*return code is %s" % (kc, row, ql.CODES[wrong])):
            checker.check(records, _edit(outs, kc, lambda a: _all_lanes(a, row, 57, 0, [wrong])))
    # the right point, out of range: X + 8 p in the four lanes
    x = value(_s32(outs[kc][1][crow, 1:15].tolist()))
    with pytest.raises(AssertionError, match=r"row %d .*X = .* lies outside" % crow):
        checker.check(records, _edit(outs, kc, lambda a: _all_lanes(a, crow, 57, 1, limbs(x + 8 * P))))
    # the negated point, for every point operation
    for name, at, lane_words in (("xyzz28_add_quad_core", 15, 57), ("xyzz28_add_quad_mem", 14, 56), ("xyzz28_dbl_quad", 14, 56), ("jac28_dbl_quad", 14, 42),
                                 ("jac28_dbl_quad/chain", 14, 42), ("xyzz28_quad_ladder", 14, 56), ("xyzz28_from_jac", 14, 56)):
        k = rec[name]
        row = crow if k == kc else 3
        y = value(_s32(outs[k][1][row, at:at + 14].tolist()))

        def negate(a):
            if name == "xyzz28_from_jac":
                a[row, at:at + 14] = _u32([limbs(-y)], 14)[0]
            else:
                _all_lanes(a, row, lane_words, at, limbs(-y))
        what = "X and Y are not the operand's limbs" if name == "xyzz28_from_jac" else "not the oracle's point"      # (from_jac hands Y on)
        with pytest.raises(AssertionError, match=r"%s record %d row %d .*%s" % (name, k, row, what)):
            checker.check(records, _edit(outs, k, negate))
    # an inverse multiplied by 2
    for name in ql.INVERSIONS:
        k = rec[name]
        row = 70 % ql.INVERSIONS[name] + ql.INVERSIONS[name]      # a lane of the second work-group
        assert any(records[k][1][row])
        if name.startswith("t_"):
            two = limbs(2 * value(_s32(outs[k][1][row].tolist())))
        else:
            two = words32(2 * _words(outs[k][1][row].tolist()) % P, 12)

        def double(a):
            a[row] = _u32([two], len(two))[0]
        with pytest.raises(AssertionError, match=r"%s record %d row %d \(work-group 1 lane %d\)" % (name, k, row, row % ql.INVERSIONS[name])):
            checker.check(records, _edit(outs, k, double))
