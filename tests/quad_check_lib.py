"""Harness of tests/device/quad_check.hip for tests/test_gpu_quad.py (gfx950 build) and tests/test_quad_check_cpu.py (no GPU): the
operation table, the rows of the quad-cooperative point formulas (curdleproofs_amd/csrc/g1_28_quad.hpp) and of the work-group
inversions (block_inverse.hpp), and the checks of every result against Python integers and, as points, against the oracle.

Rows are built on PointVectors of tests/field_check_lib.py (lazy(), xyzz(), jac(), accumulators(), records()), seeded and
deterministic.  The ORDER of the rows is part of the test: the program places rows 16 k .. 16 k + 15 of a record in one wave, so a record
either interleaves the five outcomes of an addition in every wave (mixed()) or fills whole waves with one outcome (by_outcome()).

What is asserted, in exact integer arithmetic (no tolerance):
  replication    the four lanes of a quad return bit-identical words (checked first, reported with the lane);
  return code    of xyzz28_add_quad_core, from the integers: P identity -> TAKE_Q (also when both are), else Q identity -> TAKE_P, else
                 equal points -> DOUBLE_P, else opposite points -> IDENTITY, else OK; r is looked at only under OK;
  value          every result, as a point, is the oracle's sum (PointChecks.add; chains and ladders step by step); the identity doubled
                 is the identity, xyzz28_dbl_quad of the identity returns its operand bit for bit;
  stored form    every output coordinate has limbs 0..12 in [0, 2^28) and lies in the range the headers document for an OPERAND of its
  and closure    kind (XYZZ: |X| <= 6.3 p, |Y| <= 2.7 p, ZZ and ZZZ in (-0.81 p, 1.81 p), ZZ^3 = ZZZ^2; Jacobian: |X|, |Y| <= 15.4 p,
                 |Z| <= 3.6 p), so a result is a legal next operand.  xyzz28_from_jac hands X and Y on unchanged (bit for bit, asserted),
                 so ITS result keeps the Jacobian range for X and Y, up to +-15.4 p; the kernels feed such points to the quad additions
                 and doublings (k_finalize_ranges_wave, k_msm_tail_wave), g1_28_quad.hpp documents that range as accepted, and the
                 "wide" rows of the additions and doublings feed it, at its first and last representatives too;
  inversions     table form: out z = 2^784 mod p with out normalised in (-0.81 p, 1.81 p); standard form: the words are exactly
                 z^-1 2^768 mod p.  A lane whose input is exact zero is unspecified and not compared.  A non-zero limb pattern that is
                 0 mod p is outside the functions' contract (callers pass exact zero for the identity) and is not fed."""
import random

from tests import check_harness as ch
from tests import f28_vectors as fv
from tests.check_harness import list_operations, _fmt   # noqa: F401
from tests.f28_vectors import MASK, P, R392, limbs, value
from tests.field_check_lib import PointVectors, R384, _aff_add, _jac_of, _s32, _split, _words, _xyzz_of

# ---------------------------------------------------------------- operation table: name -> (input words, output words) per row
INVERSIONS = {"t_block_batch_inverse/64": 64, "t_block_batch_inverse/256": 256, "block_batch_inverse/64": 64, "block_batch_inverse/256": 256}
TABLE = {"xyzz28_add_quad_core": (112, 4 * 57), "xyzz28_add_quad_mem": (113, 4 * 56), "xyzz28_dbl_quad": (56, 4 * 56), "jac28_dbl_quad": (42, 4 * 42),
         "jac28_dbl_quad/chain": (43, 4 * 42), "xyzz28_quad_ladder": (113, 4 * 56), "xyzz28_from_jac": (42, 56)}
TABLE.update({name: (14, 14) if name.startswith("t_") else (12, 12) for name in INVERSIONS})
QUAD_OPS = tuple(n for n, (_, no) in TABLE.items() if n not in INVERSIONS and n != "xyzz28_from_jac")
# the last input word of these rows is a parameter; the values the program accepts (else it exits with 3)
PARAMETERS = {"xyzz28_add_quad_mem": (0, 1), "jac28_dbl_quad/chain": (1, 128), "xyzz28_quad_ladder": (0, 0xffff)}

OK, TAKE_Q, TAKE_P, DOUBLE_P, IDENTITY = range(5)      # g1_28_quad.hpp
CODES = ("QUAD_OK", "QUAD_TAKE_Q", "QUAD_TAKE_P", "QUAD_DOUBLE_P", "QUAD_IDENTITY")
WAVE = 16                                               # rows per wave
COUNTS = (1, 2, 8, 56, 120)                             # 56 and 120: the chains of k_table_build_quad
PATTERNS = (0x0000, 0xffff, 0x8001, 0x5555)
# the representative of (X, Y, ZZ, ZZZ) / (X, Y, Z): all lowest, all highest, alternating
COMBOS = (("lo",) * 4, ("hi",) * 4, ("lo", "hi", "lo", "hi"), ("hi", "lo", "hi", "lo"))


def run(exe, records, work_dir, tag, timeout=120):
    return ch.run(exe, TABLE, records, work_dir, tag, timeout)


# ---------------------------------------------------------------- what the integers expect

def _neg(a):
    return None if a is None else (a[0], (-a[1]) % P)


def code_of(a, b):
    """the return code of xyzz28_add_quad_core for the points a + b (affine integers, None = the identity)"""
    if a is None:
        return TAKE_Q
    if b is None:
        return TAKE_P
    if a == b:
        return DOUBLE_P
    return IDENTITY if a == _neg(b) else OK


def add_row_code(row):
    """the expected code of a row of xyzz28_add_quad_core or (113 words, same-slot flag last) xyzz28_add_quad_mem"""
    a = _xyzz_of(row[:56])
    return code_of(a, a if len(row) == 113 and row[112] else _xyzz_of(row[56:112]))


def ladder_trace(a, q, pattern):
    """the double-and-add of xyzz28_quad_ladder on affine integers: (the code every addition meets, the final point)"""
    codes = []
    for bit in range(15, -1, -1):
        a = _aff_add(a, a)
        if (pattern >> bit) & 1:
            codes.append(code_of(a, q))
            a = _aff_add(a, q)
    return codes, a


# ---------------------------------------------------------------- rows

def mixed(rows, waves=16):
    """`waves` waves that each hold all five outcomes: the outcome of row i of a wave is i mod 5, the rows of an outcome in turn"""
    pools = {c: [r for r in rows if add_row_code(r) == c] for c in range(5)}
    assert all(pools.values())
    return [pools[i % 5][(w * 4 + i // 5) % len(pools[i % 5])] for w in range(waves) for i in range(WAVE)]


def by_outcome(rows):
    """every row, ordered so that a wave holds ONE outcome: the rows of an outcome, filled up to whole waves with its first rows"""
    out = []
    for c in range(5):
        pool = [r for r in rows if add_row_code(r) == c]
        out += pool + [pool[i % len(pool)] for i in range(-len(pool) % WAVE)]
    return out


class QuadVectors(PointVectors):
    def __init__(self, orc, seed=4300):
        super().__init__(orc, seed)
        self.seed = seed
        self.accs = self.accumulators()
        self.extreme = self.accs[1::3]      # eight accumulators with ZZ != 1 for most
        assert len(self.extreme) >= 8

    def scale(self):
        return self.rng.randrange(2, P)

    def reseed(self, what):
        """every generator draws from a stream of its own: its rows do not depend on what was generated before"""
        self.rng = random.Random("%d/%s" % (self.seed, what))

    # -- additions
    def add_rows(self):
        """every pair shape PointVectors.records() makes for xyzz28_add (generic, P + P and P - P on the same and on different ZZ,
        the identity on either and on both sides), then the extreme representatives: each of X, Y, ZZ, ZZZ of both operands at the
        lowest / highest representative of its range, for generic pairs and for P + P and P - P"""
        self.reseed("add")
        rows = list(dict(self.records())["xyzz28_add"])
        for i, (acc, a) in enumerate(self.extreme):
            acc2, a2 = self.accs[(3 * i + 8) % len(self.accs)]
            assert a2 != a and a2 != _neg(a)
            nacc = (acc[0], (-acc[1]) % P, acc[2], acc[3])
            for c1 in COMBOS:
                rows += [self.xyzz(acc, self.scale(), c1) + self.xyzz(acc2, self.scale(), c2) for c2 in COMBOS]
                rows += [self.xyzz(acc, 1, c1) + self.xyzz(other, self.scale(), c1[::-1]) for other in (acc, nacc)]
                # operands that come from xyzz28_from_jac: X and Y in the Jacobian range, +-15.4 p
                rows += [self.xyzz(acc, self.scale(), c1, wide=True) + self.xyzz(o, self.scale(), c1[::-1], wide=True) for o in (acc2, acc, nacc)]
                rows.append(self.xyzz(acc, self.scale(), c1, wide=True) + self.xyzz(acc2, self.scale(), c1, wide=True))
        return rows

    def mem_rows(self):
        """the rows of add_rows() with both operands in slots of their own, then the same-slot rows (ia == ib; the second point is
        ignored): generic points, extreme representatives and the identity"""
        rows = [r + [0] for r in self.add_rows()]
        self.reseed("mem")
        other = lambda: self.xyzz(self.rng.choice(self.accs)[0], self.scale())
        rows += [self.xyzz(acc, s) + other() + [1] for acc, _ in self.accs for s in (1, self.scale())]
        rows += [self.xyzz(acc, self.scale(), c, wide=w) + other() + [1] for acc, _ in self.extreme for c in COMBOS for w in (False, True)]
        rows += [self.xyzz(None) + other() + [1], self.xyzz(None) + self.xyzz(None) + [1]]
        return rows

    def add_records(self):
        core, mem = self.add_rows(), self.mem_rows()
        return [("xyzz28_add_quad_core", mixed(core)), ("xyzz28_add_quad_core", by_outcome(core)),
                ("xyzz28_add_quad_mem", mixed(mem)), ("xyzz28_add_quad_mem", by_outcome(mem))]

    # -- doublings
    def xyzz_rows(self):
        self.reseed("xyzz")
        rows = [self.xyzz(acc, s) for acc, _ in self.accs for s in (1, self.scale())]
        rows += [self.xyzz(acc, self.scale(), c, wide=w) for acc, _ in self.extreme for c in COMBOS for w in (False, True)]
        rows.insert(5, self.xyzz(None))      # the identity among live points, and a whole wave of it
        return rows + [self.xyzz(None)] * WAVE

    def jac_rows(self):
        self.reseed("jac")
        rows = [self.jac(acc, s) for acc, _ in self.accs for s in (1, self.scale())]
        rows += [self.jac(acc, self.scale(), c[:3]) for acc, _ in self.extreme for c in COMBOS]
        rows.insert(5, self.jac(None))
        return rows + [self.jac(None)] * WAVE

    def dbl_records(self):
        return [("xyzz28_dbl_quad", self.xyzz_rows()), ("jac28_dbl_quad", self.jac_rows())]

    def from_jac_records(self):
        return [("xyzz28_from_jac", self.jac_rows())]

    # -- chains
    def chain_records(self):
        """COUNTS doublings in registers from normalised points (x, y, 1 as k_table_build_quad starts: Jac28::from_affine) and from the
        extreme representatives of a Jacobian point; the identity runs along"""
        self.reseed("chain")
        starts = []
        for acc, a in self.extreme[:3]:
            starts.append(self.aff(a) + limbs(R392 % P))
            starts += [self.jac(acc, self.scale(), c[:3]) for c in COMBOS]
        starts.append(self.jac(None))
        return [("jac28_dbl_quad/chain", [s + [n] for n in COUNTS for s in starts])]

    def ladder_rows(self):
        """(accumulator, Q, pattern).  From the identity and from acc = Q (the first addition after a doubling meets 2 P + P) over
        PATTERNS and four random patterns; from acc = -Q with bit 15 clear and set.  Since 2 (-Q) + Q = -Q that start never meets
        P + (-P), so the starts that do meet an exceptional addition in mid-chain follow: Q = -2 acc (bit 15 set: the first addition is
        P + (-P), the chain goes on from the identity), Q = -4 acc (bit 15 clear, bit 14 set) and Q = 2 acc (the addition meets P + P)."""
        self.reseed("ladder")
        pats = list(PATTERNS) + [self.rng.randrange(1 << 16) for _ in range(4)]
        x = lambda a, c=(None,) * 4: self.xyzz(None if a is None else (a[0], a[1], 1, 1), self.scale(), c)
        rows = []
        for i, pat in enumerate(pats):
            acc, a = self.accs[(5 * i + 2) % len(self.accs)]
            rows.append(self.xyzz(None) + self.xyzz(acc, self.scale(), COMBOS[i % 4] if i >= 4 else (None,) * 4) + [pat])
            rows.append(self.xyzz(acc, self.scale()) + self.xyzz(acc, self.scale()) + [pat])
        for i, pat in enumerate((0x4000, 0x8000, 0x5555, 0xffff)):
            a = self.pts[i]
            rows.append(x(_neg(a)) + x(a) + [pat])
        for i, (k, ps) in enumerate(((-2, (0x8000, 0xffff, 0xc001)), (-4, (0x4000, 0x7fff)), (2, (0x8000, 0xffff)))):
            a = self.pts[8 + i]
            q = _aff_add(a, a)
            q = _aff_add(q, q) if abs(k) == 4 else q
            q = _neg(q) if k < 0 else q
            rows += [x(a, COMBOS[j % 4]) + x(q) + [pat] for j, pat in enumerate(ps)]
        return rows

    def ladder_records(self):
        return [("xyzz28_quad_ladder", self.ladder_rows())]

    # -- inversions
    def inverse_blocks(self, name):
        """one work-group of n lanes per pattern: [(pattern, rows)].  Table form: representatives at random of the product range and of a
        Jacobian Z (+-3.6 p, either sign); standard form: canonical Montgomery residues below p.  Zero lanes are exact zeros."""
        n, table = INVERSIONS[name], name.startswith("t_")
        self.reseed(name)
        rng = self.rng
        if table:
            rep = lambda v: self.lazy(v, *rng.choice(((-81, 181), (-360, 360))))
            zero, one = [0] * 14, limbs(R392 % P)
        else:
            rep = lambda v: fv.words32(v * R384 % P, 12)
            zero, one = [0] * 12, fv.words32(R384 % P, 12)
        val = lambda: rep(rng.randrange(1, P))
        distinct = lambda: [val() for _ in range(n)]
        blocks = [("distinct", distinct())]
        blocks += [("zero at lane %d" % z, [zero if i == z else r for i, r in enumerate(distinct())]) for z in (0, n - 1)]
        blocks += [("zero at every odd lane", [zero if i & 1 else r for i, r in enumerate(distinct())])]
        blocks += [("all zero but lane %d" % z, [r if i == z else zero for i, r in enumerate(distinct())]) for z in (0, 37, n - 1)]
        blocks += [("all zero", [zero] * n), ("all ones", [one] * n), ("equal values", [val()] * n)]
        pairs = []
        for _ in range(n // 2):
            v = rng.randrange(2, P)
            pairs += [rep(v), rep(pow(v, -1, P))]
        blocks.append(("a value next to its inverse", pairs))
        if n == 256:
            blocks.append(("a wave of zeros", [zero if 64 <= i < 128 else r for i, r in enumerate(distinct())]))
        return blocks

    def inverse_records(self, name):
        return [(name, [r for _, rows in self.inverse_blocks(name) for r in rows])]


# ---------------------------------------------------------------- checks

def _stored(coords):
    assert all(0 <= v <= MASK for c in coords for v in c[:13]), "a stored coordinate is not normalised"
    return [value(c) for c in coords]


def _within(v, lo, hi, what):
    assert lo * P <= 100 * v <= hi * P, "%s = %.3f p lies outside [%.2f p, %.2f p]" % (what, v / P, lo / 100, hi / 100)


def _product(v, what):
    assert -81 * P < 100 * v < 181 * P, "%s = %.3f p lies outside (-0.81 p, 1.81 p)" % (what, v / P)


def xyzz_operand(o, wide=False):
    """o (56 signed limbs) is a legal XYZZ operand: the range of a result of the XYZZ formulas, or (wide) with X and Y in the range of
    a Jacobian point, what xyzz28_from_jac hands on; returns its point"""
    X, Y, ZZ, ZZZ = _stored(_split(o, 14))
    _within(X, *((-1540, 1540) if wide else (-630, 630)), "X")
    _within(Y, *((-1540, 1540) if wide else (-270, 270)), "Y")
    _product(ZZ, "ZZ")
    _product(ZZZ, "ZZZ")
    assert (ZZ ** 3 - ZZZ ** 2 * R392) % P == 0, "ZZ^3 != ZZZ^2"
    return _xyzz_of(o, True)


def jac_operand(o):
    X, Y, Z = _stored(_split(o, 14))
    _within(X, -1540, 1540, "X")
    _within(Y, -1540, 1540, "Y")
    _within(Z, -360, 360, "Z")
    return _jac_of(o, True)


def _point(got, want):
    assert got == want, "not the oracle's point: %s instead of %s" % (got, want)


class Checker:
    """every output row of every record against the integers and the oracle (points: PointChecks of tests/field_check_lib.py)"""

    def __init__(self, points):
        self.points = points

    def times(self, a, k):
        """2^k a, doubling by doubling through the oracle"""
        for _ in range(k):
            a = self.points.add(a, a)
        return a

    def ladder(self, a, q, pattern):
        for bit in range(15, -1, -1):
            a = self.points.add(a, a)
            if (pattern >> bit) & 1:
                a = self.points.add(a, q)
        return a

    # each returns whether a value was compared
    def core(self, i, o):
        want = add_row_code(i)
        assert o[0] == want, "the return code is %s, the integers give %s" % (CODES[o[0]] if 0 <= o[0] < 5 else o[0], CODES[want])
        if want == OK:
            _point(xyzz_operand(o[1:]), self.points.add(_xyzz_of(i[:56]), _xyzz_of(i[56:])))
        return want == OK

    def mem(self, i, o):
        a = _xyzz_of(i[:56])
        _point(xyzz_operand(o), self.points.add(a, a if i[112] else _xyzz_of(i[56:112])))
        return True

    def dbl(self, i, o):
        a = _xyzz_of(i)
        _point(xyzz_operand(o), self.points.add(a, a))
        if a is None:
            assert o == i, "the identity doubled is not the operand bit for bit"
        return True

    def jac_dbl(self, i, o):
        a = _jac_of(i[:42])
        _point(jac_operand(o), self.times(a, i[42] if len(i) == 43 else 1))
        return True

    def ladder_row(self, i, o):
        _point(xyzz_operand(o), self.ladder(_xyzz_of(i[:56]), _xyzz_of(i[56:112]), i[112]))
        return True

    def from_jac(self, i, o):
        """X and Y pass through bit for bit (so they keep the Jacobian range: what the quad formulas accept as operands, g1_28_quad.hpp,
        and what the wide rows of the additions and doublings feed), ZZ and ZZZ are products"""
        if not any(i[28:]):
            assert o == limbs(R392 % P) * 2 + [0] * 28, "the identity is not Xyzz28::identity()"
            return True
        assert o[:28] == i[:28], "X and Y are not the operand's limbs"
        _point(xyzz_operand(o, wide=True), _jac_of(i))
        return True

    def table_inverse(self, i, o):
        if not any(i):
            return False
        z, (t,) = value(i), _stored([o])
        _product(t, "the inverse")
        assert z % P, "the row is outside the contract"
        assert (t * z - R392 * R392) % P == 0, "out z != 2^784 mod p"
        return True

    def std_inverse(self, i, o):
        if not any(i):
            return False
        want = pow(_words(i), -1, P) * R384 * R384 % P
        assert _words(o) == want, "not the canonical z^-1 2^768 mod p = %#x" % want
        return True

    def check(self, records, got, who="device"):
        """returns (rows checked, values compared); a failure names the operation, the record, the row, the lane and the limbs"""
        rows_n = compared = 0
        for k, ((name, rows), (gname, g)) in enumerate(zip(records, got)):
            assert gname == name and len(g) == len(rows), name
            if name in INVERSIONS:
                fn, lanes, signed = (self.table_inverse if name.startswith("t_") else self.std_inverse), 1, name.startswith("t_")
            else:
                fn = {"xyzz28_add_quad_core": self.core, "xyzz28_add_quad_mem": self.mem, "xyzz28_dbl_quad": self.dbl, "jac28_dbl_quad": self.jac_dbl,
                      "jac28_dbl_quad/chain": self.jac_dbl, "xyzz28_quad_ladder": self.ladder_row, "xyzz28_from_jac": self.from_jac}[name]
                lanes, signed = (4 if name in QUAD_OPS else 1), True
            for r, (row, out) in enumerate(zip(rows, g.tolist())):
                per = _split(_s32(out) if signed else out, len(out) // lanes)
                where = "%s record %d row %d (wave %d)" % (name, k, r, r // WAVE)
                if name in INVERSIONS:
                    where = "%s record %d row %d (work-group %d lane %d)" % (name, k, r, r // INVERSIONS[name], r % INVERSIONS[name])
                for lane in range(1, lanes):      # replication first
                    if per[lane] != per[0]:
                        raise AssertionError("%s lane %d: the %s result differs from lane 0's\n  in  %s\n  lane 0 %s\n  lane %d %s" % (
                            where, lane, who, _fmt(row), _fmt(per[0]), lane, _fmt(per[lane])))
                try:
                    compared += bool(fn(row, per[0]))
                except AssertionError as e:
                    raise AssertionError("%s lane 0..%d: the %s result is not what the integers give (%s)\n  in  %s\n  out %s" % (
                        where, lanes - 1, who, str(e)[:400], _fmt(row), _fmt(per[0]))) from None
                rows_n += 1
        return rows_n, compared
