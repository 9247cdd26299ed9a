"""Harness of tests/device/field_check.hip for tests/test_field_check_cpu.py (host twin, g++) and tests/test_gpu_field.py (gfx950
build): the operation table, the rows of every operation group (tests/f28_vectors.py) and the checks of
every operation's result against Python integers and, for the point formulas, against the oracle as points."""
import functools
import os
import random

from tests import check_harness as ch
from tests import f28_vectors as fv
from tests.check_harness import list_operations, read_records, assert_same, _fmt   # noqa: F401
from tests.f28_vectors import MASK, P, R392, RMOD, limbs, value, cneg_lazy, lazy_diff, check_montgomery

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "device", "field_check.hip")
R384 = 1 << 384

# ---------------------------------------------------------------- operation table: name -> (input words, output words)
BODIES3 = ("0", "1", "2", "-1")          # the numbering of tests/host_emul/f28_redc_bodies.cpp
SQR_BODIES = ("0", "2", "-1")
MIXED = ("xyzz28_add_mixed", "xyzz28_add_mixed_inl", "xyzz28_add_mixed_t/1,1,1", "xyzz28_add_mixed_t/1,1,0", "xyzz28_add_mixed_t/1,0,0",
         "xyzz28_add_mixed_t/0,0,0")
TABLE = {}
for _b in BODIES3:
    TABLE["f28_mul_body/" + _b] = (28, 14)
for _b in BODIES3:
    TABLE["f28_mul/" + _b] = (28, 14)
for _b in BODIES3:
    TABLE["f28_mulsub_body/" + _b] = (56, 14)
for _b in SQR_BODIES:
    TABLE["f28_sqr_body/" + _b] = (14, 14)
for _b in SQR_BODIES:
    TABLE["f28_sqr/" + _b] = (14, 14)
TABLE.update({"f28_normalize": (14, 14), "f28_add": (28, 14), "f28_sub": (28, 14), "f28_sub_sub2": (42, 14), "f28_neg": (14, 14),
              "f28_cneg": (15, 14), "f28_shl/1": (14, 14), "f28_shl/2": (14, 14), "f28_shl/3": (14, 14), "f28_product_is_zero": (14, 1),
              "f28_from_std": (12, 14), "f28_to_std": (14, 12), "f28_canonical_words": (14, 12), "f28_from_words": (12, 14),
              "f28_inv_euclid": (14, 14), "f28_inv": (14, 14), "f28_consts": (1, 70)})
FE_OPS = {"mul": 2, "mul_body": 2, "sqr": 1, "add": 2, "sub": 2, "neg": 1, "dbl": 1, "from_mont": 1, "to_mont": 1}
FIELDS = {"fp": (P, 12), "fr": (RMOD, 8)}
for _f, (_p, _n) in FIELDS.items():
    for _o, _k in FE_OPS.items():
        TABLE["%s_%s" % (_f, _o)] = (_k * _n, _n)
for _m in MIXED:
    TABLE[_m] = (84, 56)
TABLE.update({"xyzz28_add": (112, 56), "xyzz28_dbl": (56, 56), "xyzz28_dbl_affine": (28, 56), "xyzz28_to_jac": (56, 42), "jac28_dbl": (42, 42),
              "jac28_add_mixed": (70, 42), "jac28_add": (84, 42)})
GROUPS = ("f28_products", "f28_linear", "mont32", "points")


def group_of(name):
    if name.startswith("f28_"):
        return "f28_products" if name.partition("/")[0] in ("f28_mul_body", "f28_mul", "f28_mulsub_body", "f28_sqr_body", "f28_sqr") else "f28_linear"
    return "mont32" if name[:3] in ("fp_", "fr_") else "points"


# ---------------------------------------------------------------- building and running

build_host_twin = functools.partial(ch.build_host_twin, SRC, name="field_check_host")      # (out_dir, extra=())


def write_records(path, records):      # (tests/host_emul/sanitize.sh writes the extreme products with it)
    ch.write_records(path, TABLE, records)


def run(exe, records, work_dir, tag, timeout=120):
    return ch.run(exe, TABLE, records, work_dir, tag, timeout)


# ---------------------------------------------------------------- integer checks, one per operation

def _s32(row):
    return [x - (1 << 32) if x >= (1 << 31) else x for x in row]


def _words(row):
    return sum(x << (32 * i) for i, x in enumerate(row))


def _split(row, k):
    return [row[i:i + k] for i in range(0, len(row), k)]


def _exact(out, v):
    """the normalised limbs of the integer v: limbs 0..12 in [0, 2^28), the top limb signed; the value is exact, not only mod p"""
    assert _s32(out) == limbs(v)


def _check_inverse(inp, out):
    t = _s32(out)
    assert all(0 <= x <= MASK for x in t[:13])
    a = value(inp)
    assert -81 * P // 100 < value(t) < 181 * P // 100
    if a % P:
        assert (value(t) * a - R392 * R392) % P == 0      # a^-1 in Montgomery form
    else:
        assert value(t) % P == 0                          # 0 -> 0


def _check_consts(inp, out):
    want = [R392 % P, (1 << 400) % P, R384 % P, (1 << 1176) % P, 4 * R392 % P]
    assert [_s32(x) for x in _split(out, 14)] == [limbs(v) for v in want]


def _f28_check(name):
    op, _, body = name.partition("/")
    if op in ("f28_mul_body", "f28_mul"):
        return lambda i, o: check_montgomery(_s32(o), value(i[:14]) * value(i[14:]))
    if op == "f28_mulsub_body":
        return lambda i, o: check_montgomery(_s32(o), value(i[:14]) * value(i[14:28]) - value(i[28:42]) * value(i[42:]))
    if op in ("f28_sqr_body", "f28_sqr"):
        return lambda i, o: check_montgomery(_s32(o), value(i) ** 2)
    if op == "f28_shl":
        return lambda i, o: _exact(o, value(i) << int(body))
    return {
        "f28_normalize": lambda i, o: _exact(o, value(i)),
        "f28_add": lambda i, o: _exact(o, value(i[:14]) + value(i[14:])),
        "f28_sub": lambda i, o: _exact(o, value(i[:14]) - value(i[14:])),
        "f28_sub_sub2": lambda i, o: _exact(o, value(i[:14]) - value(i[14:28]) - 2 * value(i[28:])),
        "f28_neg": lambda i, o: _exact(o, -value(i)),
        "f28_cneg": lambda i, o: _exact(o, -value(i[:14])) if i[14] else _same(_s32(o), i[:14]),
        # value mod p == 0 on the range the header documents for a product, (-0.81 p, 1.81 p): 0 and p; no multiple beyond it
        "f28_product_is_zero": lambda i, o: _same(o, [1 if value(i) % P == 0 and -81 * P < 100 * value(i) < 181 * P else 0]),
        "f28_from_std": lambda i, o: check_montgomery(_s32(o), _words(i) * ((1 << 400) % P)),
        "f28_to_std": lambda i, o: _same(_words(o), value(i) * pow(1 << 8, -1, P) % P),
        "f28_canonical_words": lambda i, o: _same(_words(o), value(i) % P),
        "f28_from_words": lambda i, o: _exact(o, _words(i)),
        "f28_inv_euclid": _check_inverse,
        "f28_inv": _check_inverse,
        "f28_consts": _check_consts,
    }[op]


def _same(a, b):
    assert a == b, (a, b)


def _fe_check(name):
    f, _, op = name.partition("_")
    p, n = FIELDS[f]
    R, Ri = 1 << (32 * n), pow(1 << (32 * n), -1, p)
    a = lambda i: _words(i[:n])
    b = lambda i: _words(i[n:])
    want = {"mul": lambda i: a(i) * b(i) * Ri, "mul_body": lambda i: a(i) * b(i) * Ri, "sqr": lambda i: a(i) * a(i) * Ri,
            "add": lambda i: a(i) + b(i), "sub": lambda i: a(i) - b(i), "neg": lambda i: -a(i), "dbl": lambda i: 2 * a(i),
            "from_mont": lambda i: a(i) * Ri, "to_mont": lambda i: a(i) * R}[op]
    return lambda i, o: _same(_words(o), want(i) % p)      # canonical: exactly the residue below p


# points: decode as affine integers (None = identity) from the Montgomery-form lazy limbs
def _aff_of(row):
    x, y = value(row[:14]), value(row[14:])
    if not any(row):
        return None
    Ri = pow(R392, -1, P)
    return (x * Ri % P, y * Ri % P)


def _xyzz_of(row, stored=False):
    x, y, zz, zzz = (_split(row, 14))
    if not any(zz):
        return None
    if stored:
        assert all(0 <= v <= MASK for c in (x, y, zz, zzz) for v in c[:13]), "a stored coordinate is not normalised"
    x, y, zz, zzz = value(x), value(y), value(zz), value(zzz)
    assert zz % P and zzz % P and (zz ** 3 - zzz ** 2 * R392) % P == 0, "ZZ^3 != ZZZ^2"
    return (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P)


def _jac_of(row, stored=False):
    x, y, z = (_split(row, 14))
    if not any(z):
        return None
    if stored:
        assert all(0 <= v <= MASK for c in (x, y, z) for v in c[:13]), "a stored coordinate is not normalised"
    x, y, z = value(x), value(y), value(z)
    assert z % P
    zi = pow(z, -1, P)
    return (x * R392 * zi * zi % P, y * R392 * R392 * zi ** 3 % P)


class PointChecks:
    """expected sums from the oracle (its complete Jacobian addition), as affine integers"""

    def __init__(self, orc):
        self.orc = orc
        self.cache = {}

    def _jac_bytes(self, a):
        one = (R384 % P).to_bytes(48, "little")
        if a is None:
            return one + one + bytes(48)
        return (a[0] * R384 % P).to_bytes(48, "little") + (a[1] * R384 % P).to_bytes(48, "little") + one

    def add(self, a, b):
        if (a, b) not in self.cache:
            r = self.orc.g1_to_affine(self.orc.g1_add_jac(self._jac_bytes(a), self._jac_bytes(b)))
            Ri = pow(R384, -1, P)
            x, y = int.from_bytes(r[:48], "little") * Ri % P, int.from_bytes(r[48:], "little") * Ri % P
            self.cache[(a, b)] = None if r == bytes(96) else (x, y)
        return self.cache[(a, b)]

    def check(self, name):
        op = name.partition("/")[0]
        if op in ("xyzz28_add_mixed", "xyzz28_add_mixed_inl", "xyzz28_add_mixed_t"):
            return lambda i, o: _same(_xyzz_of(_s32(o), True), self.add(_xyzz_of(i[:56]), _aff_of(i[56:])))
        return {
            "xyzz28_add": lambda i, o: _same(_xyzz_of(_s32(o), True), self.add(_xyzz_of(i[:56]), _xyzz_of(i[56:]))),
            "xyzz28_dbl": lambda i, o: _same(_xyzz_of(_s32(o), True), self.add(_xyzz_of(i), _xyzz_of(i))),
            "xyzz28_dbl_affine": lambda i, o: _same(_xyzz_of(_s32(o), True), self.add(_aff_of(i), _aff_of(i))),
            "xyzz28_to_jac": lambda i, o: _same(_jac_of(_s32(o), True), _xyzz_of(i)),
            "jac28_dbl": lambda i, o: _same(_jac_of(_s32(o), True), self.add(_jac_of(i), _jac_of(i))),
            "jac28_add_mixed": lambda i, o: _same(_jac_of(_s32(o), True), self.add(_jac_of(i[:42]), _aff_of(i[42:]))),
            "jac28_add": lambda i, o: _same(_jac_of(_s32(o), True), self.add(_jac_of(i[:42]), _jac_of(i[42:]))),
        }[op]


def check_integers(records, got, points=None, who="device"):
    """every output row against Python integers (points: against the oracle); returns the number of rows checked"""
    n = 0
    for (name, rows), (_, g) in zip(records, got):
        if name.startswith("f28_"):
            chk = _f28_check(name)
        elif name[:3] in ("fp_", "fr_"):
            chk = _fe_check(name)
        else:
            chk = points.check(name)
        assert len(g) == len(rows), name
        for i, (row, out) in enumerate(zip(rows, g.tolist())):
            try:
                chk(row, out)
            except AssertionError as e:
                raise AssertionError("%s row %d: the %s result is not what the integers give (%s)\n  in  %s\n  out %s" % (
                    name, i, who, str(e)[:300], _fmt(row), _fmt(out))) from None
            n += 1
    return n


# ---------------------------------------------------------------- rows of every group

def _flat(rows):
    return [[x for ls in r for x in ls] for r in rows]


def product_records():
    sq, rows2, rows4 = fv.product_operand_sets()
    rec = [("f28_mul_body/" + b, _flat(rows2)) for b in BODIES3] + [("f28_mul/" + b, _flat(rows2)) for b in BODIES3]
    rec += [("f28_mulsub_body/" + b, _flat(rows4)) for b in BODIES3]
    rec += [("f28_sqr_body/" + b, sq) for b in SQR_BODIES] + [("f28_sqr/" + b, sq) for b in SQR_BODIES]
    return rec


def extreme_product_records():
    """the extreme-limb set alone (the host twin under UBSan runs it)"""
    e = fv.extreme_sets()
    rows2, rows4 = _flat(e["pairs"] + e["digit_rows"]), _flat(e["fours"] + e["same_sign"] + e["digit_fours"])
    rec = [("f28_mul_body/" + b, rows2) for b in BODIES3] + [("f28_mulsub_body/" + b, rows4) for b in BODIES3]
    return rec + [("f28_sqr_body/" + b, e["squares"]) for b in SQR_BODIES]


def linear_records():
    rng = random.Random(2820)
    ops = fv.linear_operands()
    pick = lambda k, n: [[x for _ in range(k) for x in rng.choice(ops)] for _ in range(n)]
    ext = ops[:16]
    rec = [("f28_normalize", fv.normalize_operands() + ops)]
    rec += [("f28_add", [a + b for a in ext for b in ext] + pick(2, 1500)), ("f28_sub", [a + b for a in ext for b in ext] + pick(2, 1500))]
    rec += [("f28_sub_sub2", [a + b + c for a in ext[10:16] for b in ext[10:16] for c in ext[10:16]] + pick(3, 1500))]
    rec += [("f28_neg", ops), ("f28_cneg", [a + [f] for a in ops for f in (0, 1)])]
    rec += [("f28_shl/%d" % k, ops) for k in (1, 2, 3)]
    rec += [("f28_product_is_zero", fv.product_is_zero_operands())]
    c = fv.conversion_operands()
    rec += [("f28_from_std", [fv.words32(v, 12) for v in c["std"]]), ("f28_to_std", c["lazy"] + c["product"]),
            ("f28_canonical_words", c["product"]), ("f28_from_words", [fv.words32(v, 12) for v in c["words"]])]
    inv = fv.inversion_operands()
    rec += [("f28_inv_euclid", inv), ("f28_inv", inv), ("f28_consts", [[0]])]
    return rec


def mont_vectors():
    return {f: fv.mont_operands(p, n, 3200 + n) for f, (p, n) in FIELDS.items()}


def mont_records(vectors=None):
    rec = []
    for f, (singles, pairs, _) in (vectors or mont_vectors()).items():
        n = FIELDS[f][1]
        two = [fv.words32(a, n) + fv.words32(b, n) for a, b in pairs]
        one = [fv.words32(a, n) for a in singles]
        rec += [("%s_%s" % (f, o), two if k == 2 else one) for o, k in FE_OPS.items()]
    return rec


# Points.  A curve point is a pair of integers (None: the identity); its table-form coordinates are Montgomery residues times
# 2^392 in ANY lazy representative the formulas document: products in (-0.81 p, 1.81 p) for table entries and ZZ / ZZZ,
# |X| <= 6.3 p, |Y| <= 2.7 p for XYZZ accumulators, |X|, |Y| <= 15.4 p and |Z| <= 3.6 p for Jacobian points.
def _aff_add(a, b):
    """affine addition on y^2 = x^3 + 4 with integers (builds accumulators; every result the tests use goes through the oracle too)"""
    if a is None or b is None:
        return b if a is None else a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        l = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        l = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (l * l - a[0] - b[0]) % P
    return (x, (l * (a[0] - x) - a[1]) % P)


def _xyzz_madd(acc, q):
    """madd-2008-s on integers mod p: (X, Y, ZZ, ZZZ) + (x, y) for distinct, non-opposite points; acc None = the identity"""
    if acc is None:
        return (q[0], q[1], 1, 1)
    X, Y, ZZ, ZZZ = acc
    pp, r = (q[0] * ZZ - X) % P, (q[1] * ZZZ - Y) % P
    assert pp
    pp2 = pp * pp % P
    ppp, qq = pp * pp2 % P, X * pp2 % P
    x3 = (r * r - ppp - 2 * qq) % P
    return (x3, (r * (qq - x3) - Y * ppp) % P, ZZ * pp2 % P, ZZZ * ppp % P)


class PointVectors:
    def __init__(self, orc, seed=4100):
        self.rng = random.Random(seed)
        Ri = pow(R384, -1, P)
        raw = orc.rng(seed).g1_affine(24)
        self.pts = [(int.from_bytes(raw[96 * i:96 * i + 48], "little") * Ri % P, int.from_bytes(raw[96 * i + 48:96 * i + 96], "little") * Ri % P)
                    for i in range(24)]

    def lazy(self, v, lo, hi, pick=None):
        """limbs of a representative of the residue v 2^392 in (lo p, hi p) (hundredths of p): at random, or (pick "lo" / "hi") the
        lowest / the highest one of the range"""
        m = v * R392 % P
        ks = [k for k in range(lo // 100 - 1, hi // 100 + 1) if lo * P < 100 * (m + k * P) < hi * P]
        return limbs(m + (self.rng.choice(ks) if pick is None else ks[0] if pick == "lo" else ks[-1]) * P)

    def aff(self, a, lazy_neg=False):
        """a table entry; lazy_neg: a given as the limb-wise negated stored y of -a (f28_cneg_lazy, the bucket loops)"""
        if a is None:
            return [0] * 28
        if lazy_neg:
            return self.lazy(a[0], -81, 181) + [-x for x in self.lazy(-a[1], -81, 181)]
        return self.lazy(a[0], -81, 181) + self.lazy(a[1], -81, 181)

    def xyzz(self, acc, scale=1, pick=(None,) * 4, wide=False):
        """an accumulator (X, Y, ZZ, ZZZ), optionally moved to the equivalent (X s^2, Y s^3, ZZ s^2, ZZZ s^3); pick: per coordinate,
        None = a representative at random, "lo" / "hi" = the lowest / highest of its documented range; wide: X and Y in the range of a
        Jacobian point, +-15.4 p (what xyzz28_from_jac hands on)"""
        if acc is None:
            return limbs(R392 % P) * 2 + [0] * 28
        X, Y, ZZ, ZZZ = acc
        s2, s3 = scale * scale % P, scale ** 3 % P
        bx, by = (1540, 1540) if wide else (630, 270)
        return (self.lazy(X * s2, -bx, bx, pick[0]) + self.lazy(Y * s3, -by, by, pick[1]) + self.lazy(ZZ * s2, -81, 181, pick[2])
                + self.lazy(ZZZ * s3, -81, 181, pick[3]))

    def jac(self, acc, scale=1, pick=(None,) * 3):
        """the Jacobian point (X ZZ, Y ZZZ, ZZ) of an accumulator: Z = ZZ; pick as for xyzz(), for X, Y and Z"""
        if acc is None:
            return limbs(R392 % P) * 2 + [0] * 14
        X, Y, ZZ, ZZZ = acc
        X, Y, Z = X * ZZ * scale * scale % P, Y * ZZZ * scale ** 3 % P, ZZ * scale % P
        return self.lazy(X, -1540, 1540, pick[0]) + self.lazy(Y, -1540, 1540, pick[1]) + self.lazy(Z, -360, 360, pick[2])

    def accumulators(self):
        """(accumulator, its affine point): sums of one to five of the oracle's points, built by mixed additions: ZZ = 1 after the
        first and ZZ != 1 from the second on"""
        out = []
        for start in range(0, 20, 4):
            acc, a = None, None
            for q in self.pts[start:start + 5]:
                acc, a = _xyzz_madd(acc, q), _aff_add(a, q)
                out.append((acc, a))
        return out

    def records(self):
        rng, pts = self.rng, self.pts
        accs = self.accumulators()
        neg = lambda a: (a[0], (-a[1]) % P)
        mixed, full, jmixed, jfull = [], [], [], []
        jaff = lambda q, ln=False: self.aff(q)     # jac28_add_mixed stores q.y as it comes: its callers negate with f28_cneg
        for acc, a in accs:
            s = rng.randrange(2, P)
            for q in (rng.choice(pts), rng.choice(pts)):                         # generic, q.y as stored and lazily negated
                mixed += [self.xyzz(acc) + self.aff(q), self.xyzz(acc) + self.aff(neg(q), lazy_neg=True)]
                jmixed += [self.jac(acc) + jaff(q), self.jac(acc, s) + jaff(neg(q))]
            # P + P, P - P (the stored and the lazily negated form of either), either side the identity
            for q, ln in ((a, False), (a, True), (neg(a), False), (neg(a), True), (None, False)):
                mixed += [self.xyzz(acc) + self.aff(q, ln), self.xyzz(acc, s) + self.aff(q, ln)]
                jmixed += [self.jac(acc) + jaff(q, ln), self.jac(acc, s) + jaff(q, ln)]
            mixed += [self.xyzz(None) + self.aff(a), self.xyzz(None) + self.aff(a, lazy_neg=True)]
            jmixed += [self.jac(None) + jaff(a), self.jac(None) + jaff(neg(a))]
            for acc2, a2 in (rng.choice(accs), rng.choice(accs)):
                if a2 != a and a2 != neg(a):
                    full.append(self.xyzz(acc) + self.xyzz(acc2, s))
                    jfull.append(self.jac(acc) + self.jac(acc2, s))
            nacc = (acc[0], (-acc[1]) % P, acc[2], acc[3])
            for other in (acc, nacc):                                            # P + P and P - P on different ZZ, and on the same
                full += [self.xyzz(acc) + self.xyzz(other, s), self.xyzz(acc, s) + self.xyzz(other), self.xyzz(acc) + self.xyzz(other)]
                jfull += [self.jac(acc) + self.jac(other, s), self.jac(acc, s) + self.jac(other), self.jac(acc) + self.jac(other)]
            full += [self.xyzz(None) + self.xyzz(acc, s), self.xyzz(acc, s) + self.xyzz(None)]
            jfull += [self.jac(None) + self.jac(acc, s), self.jac(acc, s) + self.jac(None)]
        mixed.append(self.xyzz(None) + self.aff(None))
        jmixed.append(self.jac(None) + self.aff(None))
        full.append(self.xyzz(None) + self.xyzz(None))
        jfull.append(self.jac(None) + self.jac(None))
        one = [self.xyzz(acc, s) for acc, _ in accs for s in (1, rng.randrange(2, P))] + [self.xyzz(None)]
        jone = [self.jac(acc, s) for acc, _ in accs for s in (1, rng.randrange(2, P))] + [self.jac(None)]
        affs = [self.aff(q, ln) for q in pts for ln in (False, True)]
        rec = [(m, mixed) for m in MIXED]
        rec += [("xyzz28_add", full), ("xyzz28_dbl", one), ("xyzz28_dbl_affine", affs), ("xyzz28_to_jac", one), ("jac28_dbl", jone),
                ("jac28_add_mixed", jmixed), ("jac28_add", jfull)]
        return rec


def group_records(group, orc=None):
    if group == "f28_products":
        return product_records()
    if group == "f28_linear":
        return linear_records()
    if group == "mont32":
        return mont_records()
    assert group == "points"
    return PointVectors(orc).records()
