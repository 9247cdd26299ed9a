"""Harness of tests/device/scalar_check.hip for tests/test_scalar_check_cpu.py (host twin, g++) and tests/test_gpu_scalar.py (gfx950
build): the operation table, the rows of every operation group (tests/scalar_cases.py) and the check of every operation's result
against Python integers and the contract its header documents.  No check involves the twin.  The record file format and the process
runner are those of tests/check_harness.py."""
import functools
import os

import numpy as np

from tests import check_harness as ch
from tests import scalar_cases as sc
from tests.check_harness import list_operations, read_records, assert_same, _fmt   # noqa: F401
from tests.scalar_cases import P, R, Z2, H2, HALF_BOUND, FIX_CB, fix_windows

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "device", "scalar_check.hip")

# ---------------------------------------------------------------- operation table: name -> (input words, output words)
# fix_window_digits<CB, NW> as the kernels instantiate it (kernels.hip k_msm_fix<CB, FIX_WPW>, msm_body.hpp: NW = FIX_WPW, the slices
# w0 = 0, NW, 2 NW, ...), FixDigitStream<CB> as late.hip does (k_late_fix<8 / 16 / 19>)
FIX_SLICES = ((8, 16), (8, 8), (16, 16), (16, 8), (16, 4), (16, 2), (19, 7))
TABLE = {"glv_split": (8, 10), "glv_biased_bytes": (4, 4), "recode_signed16": (8, 64), "recode_signed16/stride3": (8, 65), "recode_naf": (8, 18),
         "recode_smul_glv": (8, 20)}
for _cb in FIX_CB:
    TABLE["fix_digit_stream/%d" % _cb] = (8, fix_windows(_cb))
for _cb, _nw in FIX_SLICES:
    TABLE["fix_window_digits/%d,%d" % (_cb, _nw)] = (8, fix_windows(_cb))
TABLE.update({"recode_signed_nibbles_biased": (4, 4), "gen_recode": (8, 10), "gen_pick": (8, 64), "glv_table_entry": (8, 129),
              "tracker_ladder_step": (16, 258), "modinv30_divsteps": (3, 5), "words_inv_mod_p_divsteps": (12, 12),
              "words_inv_mod_r_divsteps": (8, 8), "fp_inv_divsteps": (12, 12), "fr_inv_divsteps": (8, 8), "fp_inv": (12, 12), "fr_inv": (8, 8),
              "fp_pow": (24, 12), "fr_pow": (16, 8), "words_inv_mod_p": (12, 12), "fp_inv_euclid": (12, 12), "fp_raw_gt": (24, 1),
              "fr_raw_gt": (16, 1)})
GROUPS = ("split", "recode", "fix", "tables", "divsteps", "inverse_p", "inverse_r")
MAX_BATCHES = {P: 40, R: 28}          # modinv30.hpp: ModInv30Cfg / ModInv30FrCfg


def group_of(name):
    op = name.partition("/")[0]
    if op in ("glv_split", "glv_biased_bytes", "gen_recode", "gen_pick", "recode_signed_nibbles_biased"):
        return "split"
    if op in ("recode_signed16", "recode_naf", "recode_smul_glv"):
        return "recode"
    if op in ("fix_digit_stream", "fix_window_digits"):
        return "fix"
    if op in ("glv_table_entry", "tracker_ladder_step"):
        return "tables"
    if op in ("modinv30_divsteps", "fp_raw_gt", "fr_raw_gt"):
        return "divsteps"
    return "inverse_r" if op.startswith("fr_") or op == "words_inv_mod_r_divsteps" else "inverse_p"


# ---------------------------------------------------------------- building and running

build_host_twin = functools.partial(ch.build_host_twin, SRC, name="scalar_check_host")      # (out_dir, extra=(), name=...)


def run(exe, records, work_dir, tag, timeout=120):
    return ch.run(exe, TABLE, records, work_dir, tag, timeout)


# ---------------------------------------------------------------- words <-> integers

def words(v, n):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def val(row):
    return sum(x << (32 * i) for i, x in enumerate(row))


def s32(x):
    return x - (1 << 32) if x >= (1 << 31) else x


def _bits(row):
    v = val(row)
    return [(v >> i) & 1 for i in range(32 * len(row))]


# ---------------------------------------------------------------- integer checks, one per operation

def _check_split(i, o):
    k, t, q, nk, nt = val(i), val(o[:4]), val(o[4:8]), o[8], o[9]
    assert nk in (0, 1) and nt in (0, 1)
    assert t < HALF_BOUND and q < HALF_BOUND and t <= H2 + 1
    v = (-t if nt else t) + q * Z2
    assert (-v if nk else v) % R == k


def _biased_digits(row):
    return [((row[w >> 2] >> (8 * (w & 3))) & 0xff) - 128 for w in range(16)]


def _check_biased_bytes(i, o):
    d = _biased_digits(o)
    assert sum(x << (8 * w) for w, x in enumerate(d)) == val(i)       # 16 digits in [-128, 127], nothing carried out of the top one


def _check_signed16(i, o):
    d = [s32(x) for x in o[:64]]
    assert all(-7 <= x <= 8 for x in d) and sum(x << (4 * w) for w, x in enumerate(d)) == val(i)
    if len(o) == 65:
        assert o[64] == 126                                              # the slots between the strided digits are untouched


def _naf_digits(nz, ng, top=None):
    """digits of the masks nz / ng after the NAF rules: ng inside nz, no two adjacent non-zero digits"""
    z, g = _bits(nz), _bits(ng)
    assert all(a or not b for a, b in zip(z, g)), "ng is not inside nz"
    assert not any(z[j] and z[j + 1] for j in range(len(z) - 1)), "adjacent non-zero digits"
    if top is not None:
        assert not any(z[top + 1:]), "a digit above bit %d" % top
    return [(-1 if b else 1) if a else 0 for a, b in zip(z, g)]


def _check_naf(i, o):
    d = _naf_digits(o[:9], o[9:], top=256)
    assert sum(x << j for j, x in enumerate(d)) == val(i)


def _smul_digits(o):
    """the two digit streams of a SmulNaf row (nz[0], nz[1], ng[0], ng[1]); none above bit 127: both halves are below 2^127, and the
    form of such a value has at most 128 digits (bit 128, word 4, stays empty)"""
    return _naf_digits(o[0:5], o[10:15], top=127), _naf_digits(o[5:10], o[15:20], top=127)


def _check_smul_glv(i, o):
    dt, dq = _smul_digits(o)
    t, q = sum(x << j for j, x in enumerate(dt)), sum(x << j for j, x in enumerate(dq))
    assert abs(t) <= H2 + 1 and abs(q) < HALF_BOUND
    assert (t + q * Z2) % R == val(i)


def _check_fix(cb):
    def chk(i, o):
        d = [s32(x) for x in o]
        assert len(d) == fix_windows(cb) and all(-(1 << (cb - 1)) <= x < (1 << (cb - 1)) for x in d)
        assert sum(x << (cb * w) for w, x in enumerate(d)) == val(i)    # exactly: nothing is carried out of the top window
    return chk


def _check_nibbles(i, o):
    d = [((o[j >> 3] >> (4 * (j & 7))) & 15) - 7 for j in range(32)]
    assert all(-7 <= x <= 8 for x in d) and sum(x << (4 * j) for j, x in enumerate(d)) == val(i)


def _check_gen_recode(i, o):
    t, q = (sum(x << (8 * w) for w, x in enumerate(_biased_digits(o[4 * h:4 * h + 4]))) for h in (0, 1))
    assert o[8] in (0, 1) and o[9] in (0, 1)
    for h in (0, 1):
        assert 0 <= _biased_digits(o[4 * h:4 * h + 4])[15] <= 0x56      # gen_table.hpp: GEN_TOP_DIGIT_MAX, never negative
    assert 0 <= t <= H2 + 1 and 0 <= q < HALF_BOUND
    assert ((-t if o[8] else t) + (-q if o[9] else q) * Z2) % R == val(i)


def _check_gen_pick(i, o):
    """the 32 picks (index, neg) add up to the scalar: entry index = 128 w + j - 1 is the multiple j 256^w, half 1 times z^2"""
    total = 0
    for h in (0, 1):
        for w in range(16):
            idx, neg = s32(o[2 * (16 * h + w)]), o[2 * (16 * h + w) + 1]
            assert neg in (0, 1)
            if idx < 0:
                assert idx == -1
                continue
            assert idx // 128 == w and 1 <= idx % 128 + 1 <= (0x56 if w == 15 else 128) and idx < 15 * 128 + 0x56
            total += (-1 if neg else 1) * (idx % 128 + 1) * (1 << (8 * w)) * (Z2 if h else 1)
    assert total % R == val(i)


ENTRY_DIGITS = {-1: (0, 0), 0: (1, 0), 1: (-1, 0), 2: (0, 1), 3: (0, -1), 4: (1, 1), 5: (-1, -1), 6: (1, -1), 7: (-1, 1)}   # tracker_ladder.hpp


def _entries_value(entries):
    return sum((ENTRY_DIGITS[e][0] + ENTRY_DIGITS[e][1] * Z2) << j for j, e in enumerate(entries)) % R


def _check_table_entry(i, o):
    e = [s32(x) for x in o]
    assert all(-1 <= x <= 7 for x in e) and _entries_value(e) == val(i)


def _check_ladder(i, o):
    e = [s32(x) for x in o]
    assert all(-1 <= x <= 7 for x in e)
    assert _entries_value(e[0::2]) == val(i[:8]) and _entries_value(e[1::2]) == val(i[8:])


def divsteps30(eta, f, g):
    """the 30-step batch of modinv30.hpp restated on integers, one division step at a time: (eta', (u, v, q, r), f', g') with
    (u f + v g, q f + r g) = 2^30 (f', g')"""
    u, v, q, r = 1, 0, 0, 1
    for _ in range(30):
        if eta < 0 and g & 1:
            eta, f, g, u, v, q, r = -eta, g, -f, q, r, -u, -v
        if g & 1:
            g, q, r = g + f, q + u, r + v
        g >>= 1
        u, v = 2 * u, 2 * v
        eta -= 1
    return eta, (u, v, q, r), f, g


def _check_divsteps(i, o):
    eta, f0, g0 = s32(i[0]), i[1], i[2]
    e1, u, v, q, r = (s32(x) for x in o)
    assert all(abs(x) <= 1 << 30 for x in (u, v, q, r))
    assert (u * f0 + v * g0) % (1 << 30) == 0 and (q * f0 + r * g0) % (1 << 30) == 0
    we, wt, wf, wg = divsteps30(eta, f0, g0)
    assert (e1, (u, v, q, r)) == (we, wt)
    assert (u * f0 + v * g0) >> 30 == wf and (q * f0 + r * g0) >> 30 == wg


def _check_words_inverse(p):
    def chk(i, o):
        a, x = val(i), val(o)
        assert x < p and (a * x % p == 1 if a else x == 0)
    return chk


def _check_mont_inverse(p, n):
    rr = (1 << (32 * n)) ** 2 % p

    def chk(i, o):
        a, x = val(i), val(o)
        assert x < p and (a * x % p == rr if a else x == 0)              # canonical; (a R)^-1 R^2, 0 -> 0
    return chk


def _check_pow(p, n):
    def chk(i, o):
        a, e = val(i[:n]), val(i[n:])
        assert val(o) == pow(a, e, p) * pow(1 << (32 * n), 1 - e, p) % p    # (A R)^e R^(1 - e) = A^e R
    return chk


def _check_gt(n):
    return lambda i, o: _same(o, [1 if val(i[:n]) > val(i[n:]) else 0])


def _same(a, b):
    assert a == b, (a, b)


def checker(name):
    op, _, arg = name.partition("/")
    if op in ("fix_digit_stream", "fix_window_digits"):
        return _check_fix(int(arg.split(",")[0]))
    return {
        "glv_split": _check_split, "glv_biased_bytes": _check_biased_bytes, "recode_signed16": _check_signed16, "recode_naf": _check_naf,
        "recode_smul_glv": _check_smul_glv, "recode_signed_nibbles_biased": _check_nibbles, "gen_recode": _check_gen_recode,
        "gen_pick": _check_gen_pick, "glv_table_entry": _check_table_entry, "tracker_ladder_step": _check_ladder,
        "modinv30_divsteps": _check_divsteps, "words_inv_mod_p_divsteps": _check_words_inverse(P), "words_inv_mod_r_divsteps": _check_words_inverse(R),
        "words_inv_mod_p": _check_words_inverse(P), "fp_inv_divsteps": _check_mont_inverse(P, 12), "fr_inv_divsteps": _check_mont_inverse(R, 8),
        "fp_inv": _check_mont_inverse(P, 12), "fr_inv": _check_mont_inverse(R, 8), "fp_inv_euclid": _check_mont_inverse(P, 12),
        "fp_pow": _check_pow(P, 12), "fr_pow": _check_pow(R, 8), "fp_raw_gt": _check_gt(12), "fr_raw_gt": _check_gt(8),
    }[op]


def check_integers(records, got, who="device"):
    """every output row against Python integers; returns the number of rows checked"""
    n = 0
    for (name, rows), (_, g) in zip(records, got):
        chk = checker(name)
        assert len(g) == len(rows), name
        for i, (row, out) in enumerate(zip(rows, g.tolist())):
            try:
                chk(row, out)
            except AssertionError as e:
                raise AssertionError("%s row %d: the %s result is not what the integers give (%s)\n  in  %s\n  out %s" % (
                    name, i, who, str(e)[:300], _fmt(row), _fmt(out))) from None
            n += 1
    return n


def check_across(records, got, who="device"):
    """what two operations say about the same rows: every slice form of fix_window_digits equals the digit stream; gen_pick follows the
    digits of gen_recode; glv_table_entry and both bases of tracker_ladder_step follow the digits of recode_smul_glv.  Returns the
    number of rows compared."""
    by = {name: (rows, g) for (name, rows), (_, g) in zip(records, got)}
    n = 0

    def rows_equal(a, b, what):
        assert by[a][0] == by[b][0], what
        if not np.array_equal(what_of(a), what_of(b)):
            i = int(np.nonzero((what_of(a) != what_of(b)).any(axis=1))[0][0])
            raise AssertionError("%s row %d: the %s result differs from %s\n  in  %s" % (a, i, who, b, _fmt(by[a][0][i])))
        return len(by[a][0])

    what_of = lambda name: by[name][1][:, :64] if name.startswith("recode_signed16") else by[name][1]
    for cb, nw in FIX_SLICES:
        a, b = "fix_window_digits/%d,%d" % (cb, nw), "fix_digit_stream/%d" % cb
        if a in by and b in by:
            n += rows_equal(a, b, "same rows")
    if "recode_signed16" in by and "recode_signed16/stride3" in by:
        n += rows_equal("recode_signed16/stride3", "recode_signed16", "same rows")
    if "gen_recode" in by and "gen_pick" in by:
        assert by["gen_recode"][0] == by["gen_pick"][0]
        for i, (d, pk) in enumerate(zip(by["gen_recode"][1].tolist(), by["gen_pick"][1].tolist())):
            for h in (0, 1):
                for w, digit in enumerate(_biased_digits(d[4 * h:4 * h + 4])):
                    want = [(128 * w + abs(digit) - 1) & 0xffffffff if digit else 0xffffffff, int((digit < 0) != bool(d[8 + h]))]
                    assert pk[2 * (16 * h + w):2 * (16 * h + w) + 2] == want, "gen_pick row %d half %d window %d: %s\n  in  %s" % (i, h, w, who, _fmt(by["gen_pick"][0][i]))
            n += 1
    if "recode_smul_glv" in by:
        want = {}
        for row, o in zip(by["recode_smul_glv"][0], by["recode_smul_glv"][1].tolist()):
            dt, dq = _smul_digits(o)
            inv = {v: k for k, v in ENTRY_DIGITS.items()}
            want[tuple(row)] = [inv[(dt[j], dq[j])] for j in range(129)]
        if "glv_table_entry" in by:
            for i, (row, o) in enumerate(zip(*(by["glv_table_entry"][0], by["glv_table_entry"][1].tolist()))):
                assert [s32(x) for x in o] == want[tuple(row)], "glv_table_entry row %d: %s\n  in  %s" % (i, who, _fmt(row))
                n += 1
        if "tracker_ladder_step" in by:
            for i, (row, o) in enumerate(zip(*(by["tracker_ladder_step"][0], by["tracker_ladder_step"][1].tolist()))):
                e = [s32(x) for x in o]
                assert e[0::2] == want[tuple(row[:8])] and e[1::2] == want[tuple(row[8:])], "tracker_ladder_step row %d: %s\n  in  %s" % (i, who, _fmt(row))
                n += 1
    return n


def across_count(group, records):
    """the number of rows check_across must have compared for a group's records"""
    return {"split": len(records[0][1]), "recode": len(records[0][1]), "fix": len(FIX_SLICES) * len(records[0][1]), "tables": 2 * len(records[1][1]),
            "divsteps": 0, "inverse_p": 0, "inverse_r": 0}[group]


# ---------------------------------------------------------------- rows of every group

_CACHE = {}


def case_sets():
    if not _CACHE:
        s = sc.scalar_cases()
        h = sc.half_cases(s)
        _CACHE.update(scalars=s, halves=h, naf=sc.naf_cases(s, h), inv_p=sc.inversion_inputs(P, 381, sc.HIGH_COUNT_P, n_random=600),
                      inv_r=sc.inversion_inputs(R, 255, sc.HIGH_COUNT_R, n_random=600), divsteps=sc.divsteps_rows())
    return _CACHE


def ladder_scalars():
    """about 1 500 scalars for the 129-step tables: the directed ones first"""
    s = case_sets()["scalars"]
    return s[:900] + s[-600:]


def group_records(group):
    c = case_sets()
    k8 = [words(v, 8) for v in c["scalars"]]
    h4 = [words(v, 4) for v in c["halves"]]
    if group == "split":
        return [("glv_split", k8), ("glv_biased_bytes", [words(v, 4) for v in c["halves"] if v <= sc.BIASED_MAX]), ("recode_signed_nibbles_biased", h4), ("gen_recode", k8), ("gen_pick", k8)]
    if group == "recode":
        return [("recode_signed16", k8), ("recode_signed16/stride3", k8), ("recode_naf", [words(v, 8) for v in c["naf"]]), ("recode_smul_glv", k8)]
    if group == "fix":
        return [("fix_digit_stream/%d" % cb, k8) for cb in FIX_CB] + [("fix_window_digits/%d,%d" % s, k8) for s in FIX_SLICES]
    if group == "tables":
        ls = ladder_scalars()
        l8 = [words(v, 8) for v in ls]
        pairs = [words(a, 8) + words(b, 8) for a, b in zip(ls, ls[7:] + ls[:7])]
        return [("recode_smul_glv", l8), ("glv_table_entry", l8), ("tracker_ladder_step", pairs)]
    if group == "divsteps":
        import random
        rng = random.Random(77)
        gt = []
        for p, n in ((P, 12), (R, 8)):
            vals = [0, 1, p - 1, p, (1 << (32 * n)) - 1, 1 << 32, (1 << 32) - 1, 1 << (32 * (n - 1)), (1 << (32 * (n - 1))) - 1] + [rng.randrange(1 << (32 * n)) for _ in range(40)]
            rows = [words(a, n) + words(b, n) for a in vals for b in vals]
            rows += [words(a, n) + words(a ^ (1 << rng.randrange(32 * n)), n) for a in vals for _ in range(8)]     # one differing bit, any word
            gt.append(rows)
        return [("modinv30_divsteps", [[eta & 0xffffffff, f, g] for eta, f, g in c["divsteps"]]), ("fp_raw_gt", gt[0]), ("fr_raw_gt", gt[1])]
    if group in ("inverse_p", "inverse_r"):
        import random
        p, n, f = (P, 12, "fp") if group == "inverse_p" else (R, 8, "fr")
        rng = random.Random(78 + n)
        inv = [words(v, n) for v in c["inv_p" if p == P else "inv_r"]]
        exps = [0, 1, 2, 3, p - 2, p - 1, p, (p - 1) // 2, (1 << (32 * n)) - 1, 1 << (32 * n - 1), 1 << 32, (1 << 32) - 1]
        bases = [0, 1, 2, p - 1, (1 << (32 * n)) % p] + [rng.randrange(p) for _ in range(5)]
        pw = [words(a, n) + words(e, n) for a in bases for e in exps] + [words(rng.randrange(p), n) + words(rng.randrange(1 << rng.randrange(1, 32 * n + 1)), n) for _ in range(200)]
        rec = [("words_inv_mod_%s_divsteps" % f[1] if f == "fr" else "words_inv_mod_p_divsteps", inv), (f + "_inv_divsteps", inv), (f + "_inv", inv[:500] + inv[-100:]),
               (f + "_pow", pw)]
        if p == P:
            assert not any(inv[0]) and all(any(r) for r in inv[1:])
            rec += [("words_inv_mod_p", inv[1:]), ("fp_inv_euclid", inv[1:])]    # mont32.hpp: 0 < a < p (0 is invalid there, only bounded)
        return rec
    raise AssertionError(group)
