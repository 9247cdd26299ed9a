"""The cases of the MSM wave check (tests/device/msm_check.hip), defined once for tests/test_msm_check_cpu.py and
tests/test_gpu_msm_waves.py.  Everything here is a Python integer, a list or a dict; nothing looks at the code under test, and no
group element appears: a table entry is a TAG (an index into a pool of unrelated points, tests/msm_check_lib.py), bit 31 for the negated
point, NONE for the identity.  A tagged table gives entry (copy c, index i) a tag of its own instead of 2^(8c) P_i, so that the content of
a bucket names every table address that went into it.

Constants restated from the comments of curdleproofs_amd/csrc/msm_body.hpp, recode.hpp and kernels.h."""
import random

from tests.scalar_cases import R, Z2, H2, Q_MAX, EDGE_SCALARS, py_split

NONE = 0xffffffff
NEG = 1 << 31
CANONICAL = 1                     # kernels.h MSM_SCALARS_CANONICAL
TBW_CAP, ROUND_PTS, ROUND_PTS_PERWIN, FIX_CHUNK = 8704, 1024, 4096, 256
POOL = 4096                       # unrelated points (drawing one costs the oracle half a millisecond); larger tables wrap around, see Tags

# the forms the library launches (kernels.hip): name of the operation -> kind, windows per wave, PERWIN, segments
FORMS = {"tblw/%d" % w: ("tblw", w, False, 1) for w in (2, 4, 8, 16, 32)}
FORMS["tblw/2,perwin"] = ("tblw", 2, True, 1)
FORMS.update({"tblw2/%d" % w: ("tblw2", w, False, 2) for w in (2, 4, 8, 16, 32)})
FORMS["pair"] = ("pair", 2, True, 1)
SORTS = {"sort/%d,0,128" % w: (w, False, 128, False) for w in (2, 4, 8, 16, 32)}
SORTS.update({"sort/16,0,256": (16, False, 256, False), "sort/32,0,256": (32, False, 256, False), "sort/2,1,128": (2, True, 128, False),
              "sort/2,1,128,digits": (2, True, 128, True)})
FIX_FORMS = {"fix/%d,%d" % f: f for f in ((16, 16), (16, 8), (16, 4), (16, 2), (8, 16), (8, 8), (19, 7))}
ALL_TBLW = [f for f in FORMS if f != "pair"]


def form_copies(form):
    kind, _, perwin, segs = FORMS[form]
    return 2 if perwin else 16 if segs == 2 else 32


# ---------------------------------------------------------------- scalars with chosen digits

def digits_value(d):
    return sum(x << (8 * w) for w, x in enumerate(d))


def from_digits(dt, dq, neg_t=0, neg_k=0):
    """the scalar k = +-(+-|t| + q z^2) whose halves have the signed radix-256 digits dt, dq (16 each, in [-128, 127]); the top digits are
    small enough that |t| <= z^2 / 2 and k' <= (r - 1) / 2, which the assertions check"""
    t, q = digits_value(dt), digits_value(dq)
    assert 0 <= t < H2 and 0 <= q <= Q_MAX and all(-128 <= x <= 127 for x in list(dt) + list(dq))
    kk = (-t if neg_t else t) + q * Z2
    assert 0 <= kk <= (R - 1) // 2 and (t or not neg_t)
    k = (R - kk) % R if neg_k else kk
    assert py_split(k)[:2] == (t, q)
    return k


def with_negations(ks):
    return [v for k in ks for v in (k, (R - k) % R)]


def random_digit_scalars(rng, n):
    out = []
    for _ in range(n):
        dt = [rng.randrange(-128, 128) for _ in range(15)] + [rng.randrange(1, 0x40)]
        dq = [rng.randrange(-128, 128) for _ in range(15)] + [rng.randrange(1, 0x40)]
        out.append(from_digits(dt, dq, rng.randrange(2), rng.randrange(2)))
    return out


def equal_window_scalar(d, neg_t=0, neg_k=0):
    """every one of the 32 windows holds the digit d (0 < d < 0x40: also the top ones)"""
    return from_digits([d] * 16, [d] * 16, neg_t, neg_k)


def edge_digit_scalars():
    """digits +-1 and -128 / 127 (buckets 0, 126 and 127) and +-64, +-65 (the set boundary 63 / 64) in every window below the top one"""
    out = []
    for d in (1, -1, 127, -128, 64, -64, 65, -65):
        for nt in (0, 1):
            out.append(from_digits([d] * 15 + [2], [d] * 15 + [2], nt, 0))
    out.append(from_digits([1, -1, 127, -128, 64, -64, 65, -65, 1, -1, 127, -128, 64, -64, 65, 3], [-128, 127, -65, 65, -64, 64, -1, 1] + [1, -1, 127, -128, 64, -64, 65, 3]))
    return out


SIGN_TURNS = [EDGE_SCALARS[k] for k in ("0", "1", "r-1", "(r-1)/2", "(r+1)/2", "z2", "z2-1", "z2+1", "z2/2", "z2/2-1", "z2/2+1", "r-z2", "qmax z2", "r - z2/2",
                                         "r - z2/2 - 1", "r - qmax z2")]


def mixed_scalars(n, seed):
    """n scalars: the edge digits, the sign turns of tests/scalar_cases.py (the all-zero scalar among them), one scalar with every window
    equal, random digits, and the negations of them all"""
    rng = random.Random(seed)
    directed = edge_digit_scalars() + SIGN_TURNS + [equal_window_scalar(5)]
    ks = with_negations(directed + random_digit_scalars(rng, max(0, n // 2 - len(directed)) + 1))
    rng.shuffle(ks)
    out = ks[:n]
    if n > 40 and 0 not in out:
        out[0] = 0
    return out


def random_scalars(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


# ---------------------------------------------------------------- tagged tables and tasks

class Tags:
    """hands out fresh tags: entry e of a case's tables gets tag e mod POOL.  Two addresses share a tag only POOL entries apart, never the
    same index of a neighbouring copy, a neighbouring index, or the same address of another segment or task: a read from a wrong address
    goes unnoticed only if it lands exactly a multiple of POOL entries away"""

    def __init__(self):
        self.next = 0

    def fresh(self, n):
        out = [(self.next + i) % POOL for i in range(n)]
        self.next += n
        return out


def seg(table, n, stride=None, off=0, idx=None):
    return dict(table=table, n=n, stride=n if stride is None else stride, off=off, idx=idx)


def task(scalars, segs, pad=0, canonical=True, digits=False):
    assert sum(s["n"] for s in segs) == len(scalars)
    segs = list(segs) + [seg(0, 0, 0)] * (2 - len(segs))
    return dict(scalars=list(scalars), segs=segs, pad=pad, canonical=canonical, digits=digits)


def plain_case(name, form, scalars, slices=1, reaches="", **kw):
    """one task over one fully tagged table of form_copies(form) copies"""
    n, tg = len(scalars), Tags()
    return dict(name=name, form=form, slices=slices, tables=[tg.fresh(form_copies(form) * max(n, 1))], tasks=[task(scalars, [seg(0, n, max(n, 1))], **kw)], reaches=reaches)


def two_segment_case(name, form, idx_on, seed, canonical=True, digits=False):
    """seg[0].n = 70 and seg[1].n = 50: the boundary lies inside the second slab.  Both tables are wider than their segments (copy_stride
    90 and 77), start at an offset, and the segments flagged in idx_on read through a gather list that reverses and repeats indices."""
    rng, tg, copies = random.Random(seed), Tags(), form_copies(form)
    tables = [tg.fresh(3 + copies * 90), tg.fresh(7 + copies * 77)]
    i0 = [rng.randrange(90) for _ in range(70)] if 0 in idx_on else None
    i1 = [76 - (i % 77) for i in range(50)] if 1 in idx_on else None
    t = task(mixed_scalars(120, seed), [seg(0, 70, 90, 3, i0), seg(1, 50, 77, 7, i1)], pad=11, canonical=canonical, digits=digits)
    return dict(name=name, form=form, slices=1, tables=tables, tasks=[t], reaches="two segments, boundary inside a slab, copy_stride > n, idx on %s" % (idx_on,))


def exceptional_case(name, form):
    """tagged tables repeat a tag: points 0 and 1 are the same table point (a doubling inside the mixed addition), point 2 its negation
    (the bucket returns to the identity) and point 3 goes on from there; point 4 is the identity entry; all five share one scalar, so they
    meet in every bucket that scalar reaches.  Points 5.. repeat the pattern P, -P alone: buckets that end as the identity."""
    copies, tg, n = form_copies(form), Tags(), 9
    rows = [tg.fresh(n) for _ in range(copies)]
    for r in rows:
        r[1] = r[0]
        r[2] = r[0] | NEG
        r[4] = NONE
        r[6] = r[5] | NEG
        r[8] = r[7]
    k1, k2, k3 = from_digits([3, -7, 64, 65, -128, 127, 1, -1, 3, -7, 64, 65, -128, 127, 1, 2], [9, -9, 100, -100, 34, 5, 6, 7] * 2), equal_window_scalar(0x21, 1, 1), equal_window_scalar(0x11)
    return dict(name=name, form=form, slices=1, tables=[[t for r in rows for t in r]], tasks=[task([k1] * 5 + [k2] * 2 + [k3] * 2, [seg(0, n)], pad=2)],
                reaches="P + P, P - P and the identity entry inside a bucket")


def small_digit_scalars(n, digit_of, seed):
    """scalars below 128 or their negations: one nonzero window (window 0 of |t|), digit digit_of(i)"""
    rng = random.Random(seed)
    return [(R - digit_of(i)) % R if rng.randrange(2) else digit_of(i) for i in range(n)]


def tblw_cases():
    cs = []
    # every form at slices 1 and 4: 100 points in 4 slices are 64 + 36 + 0 + 0 (two EMPTY slices: their sets must be identities)
    for f in ALL_TBLW:
        for sl in (1, 4):
            cs.append(plain_case("mixed100/s%d" % sl, f, mixed_scalars(100, 7), slices=sl, pad=5, reaches="edge digits, sign turns, zero scalar" + (", two empty slices" if sl == 4 else "")))
    # 257 points in 2 slices: 192 + 65
    for f in ("tblw/8", "tblw2/32", "tblw/2,perwin"):
        cs.append(plain_case("mixed257/s2", f, mixed_scalars(257, 8), slices=2, pad=1, reaches="two slices, the second ending in a one-point slab"))
    # a round that ends at TBW_CAP: 600 scalars with all 32 windows nonzero, 32 windows per wave: 2048 entries per slab, rounds of 256, 256, 88
    rng = random.Random(9)
    full = [from_digits([rng.choice((-1, 1)) * rng.randrange(1, 128) for _ in range(15)] + [rng.randrange(1, 0x40)],
                        [rng.choice((-1, 1)) * rng.randrange(1, 128) for _ in range(15)] + [rng.randrange(1, 0x40)], rng.randrange(2), rng.randrange(2)) for _ in range(600)]
    for f in ("tblw/32", "tblw2/32", "tblw/16"):
        cs.append(plain_case("cap600", f, full, reaches="rounds ending at TBW_CAP, the last one partial"))
    # a round that ends at the 10-bit point index: 1024 + 64 + 1 scalars with one nonzero window.  Round 1 fills every bin but 76 (digit
    # 77 is left out), round 2 (65 points) uses the digits 3, 77 and 128 only: most bins are empty there and keep the parked accumulators
    # of round 1, bin 76 is empty in round 1 and filled in round 2
    def d1089(i):
        if i < 1024:
            d = i % 127 + 1
            return d if d != 77 else 78
        return (3, 77, 3)[i % 3]
    for f in ("tblw/2", "tblw/32", "tblw2/16"):
        cs.append(plain_case("roundpts1089", f, small_digit_scalars(1089, d1089, 10), reaches="round of exactly 1024 points (index 1023), later round with empty bins"))
    # the PERWIN limit: 4096 + 1 points, two entries per point and wave at most
    cs.append(plain_case("perwin4097", "tblw/2,perwin", random_scalars(4097, 11), reaches="PERWIN round of 4096 points (index 4095)"))
    cs.append(plain_case("perwin4097/digits", "tblw/2,perwin", random_scalars(4097, 12), digits=True, reaches="the same with task.digits"))
    # ntot = 1, 63, 64, 65
    for n in (1, 63, 64, 65):
        for f in ("tblw/4", "tblw/2,perwin", "tblw2/8"):
            cs.append(plain_case("n%d" % n, f, mixed_scalars(n, 20 + n), reaches="ntot = %d" % n))
    # every window equal: one bin takes a whole round
    eq = [equal_window_scalar(5, i & 1, (i >> 1) & 1) for i in range(300)]
    for f in ("tblw/32", "tblw/2"):
        cs.append(plain_case("equal300", f, eq, reaches="one bin takes every entry of a round"))
    # two segments with gather lists, Montgomery and canonical scalars
    for f in ("tblw/8", "tblw2/16", "tblw/2", "tblw/2,perwin"):
        cs.append(two_segment_case("seg70+50/idx0", f, (0,), 30))
        cs.append(two_segment_case("seg70+50/idx1/mont", f, (1,), 31, canonical=False))
        cs.append(two_segment_case("seg70+50/idx01", f, (0, 1), 32, digits=f.endswith("perwin")))
    for f in ALL_TBLW:
        cs.append(exceptional_case("exceptional", f))
    return cs


def pair_case(name, scalars, reaches, digits=False, npairs=1):
    n, tg, tables, tasks = len(scalars), Tags(), [], []
    for p in range(2 * npairs):
        tables.append(tg.fresh(5 * p + 2 * (n + 3)))
        tasks.append(task(scalars, [seg(p, n, n + 3, 5 * p)], pad=100 * p + 7 * (p & 1), digits=digits))
    return dict(name=name, form="pair", slices=1, tables=tables, tasks=tasks, reaches=reaches)


def tie_scalars():
    """128 scalars, scalar i with the digit of magnitude i + 1 in the windows 0..14 of both halves: every bucket of the waves 0..14 holds
    exactly two entries, so every lane's bucket pair has the same size (every rank is a tie)"""
    return [from_digits([d] * 15 + [1], [d] * 15 + [1], i & 1, (i >> 1) & 1) for i, d in enumerate(list(range(1, 128)) + [-128])]


def pair_cases():
    cs = [pair_case("pair/mixed100", mixed_scalars(100, 40), "two pairs: different tagged bases and pads", npairs=2),
          pair_case("pair/mixed100/digits", mixed_scalars(100, 41), "the same with task.digits", digits=True),
          pair_case("pair/ties", tie_scalars(), "every lane's bucket pair has the same size"),
          pair_case("pair/longest", [equal_window_scalar(7, i & 1, (i >> 1) & 1) for i in range(150)] + random_scalars(50, 42), "one lane's pair is far the longest"),
          pair_case("pair/n4097", random_scalars(4097, 43), "two rounds")]
    ex = exceptional_case("pair/exceptional", "pair")
    tg = Tags()
    tg.next = 500
    other = tg.fresh(len(ex["tables"][0]))
    ex["tables"].append(other)
    ex["tasks"].append(task(ex["tasks"][0]["scalars"], [seg(1, 9)], pad=40))
    cs.append(ex)
    return cs


# ---------------------------------------------------------------- sort cases: (name, scalars, first, ntot, canonical)

def sort_cases(op):
    wpw, perwin, nbins, digits = SORTS[op]
    cs = [("mixed100", mixed_scalars(100, 50), 0, 100, True), ("slice64..100/mont", mixed_scalars(100, 51), 64, 100, False), ("empty slice", mixed_scalars(100, 52), 100, 100, True),
          ("ties", tie_scalars(), 0, 128, True)]
    for n in (1, 63, 64, 65):
        cs.append(("n%d" % n, mixed_scalars(n, 53 + n), 0, n, True))
    if perwin:
        cs.append(("perwin4097", random_scalars(4097, 54), 0, 4097, True))
    else:
        cs.append(("roundpts1089", small_digit_scalars(1089, lambda i: i % 127 + 1, 55), 0, 1089, True))
        if wpw >= 16:
            c = [c for c in tblw_cases() if c["name"] == "cap600"][0]
            cs.append(("cap600", c["tasks"][0]["scalars"], 0, 600, True))
    return cs


# ---------------------------------------------------------------- fixed-base cases

def fix_scalars(cb, n, seed):
    rng = random.Random(seed)
    w = -(-256 // cb)
    half = 1 << (cb - 1)
    ks = [0, 1, R - 1] + [half << (cb * j) for j in range(w) if (half << (cb * j)) < R]     # digit -2^(cb-1) in window j (and +1 above it)
    ks += [sum(half << (cb * j) for j in range(0, 255 // cb, 2))]
    ks += [rng.randrange(R) for _ in range(max(0, n - len(ks)))]
    rng.shuffle(ks)
    ks = ks[:n]
    if n >= 3:
        ks[1] = half                                                                        # window 0 = -2^(cb-1)
    return ks


def fix_cases(op):
    """tasks of one launch: (n, off, idx, canonical).  nc = 4 columns; gather lists reach them all, `off` without a list only where
    off + n <= nc."""
    cb, wpw = FIX_FORMS[op]
    rng = random.Random(60 + cb + wpw)
    tasks = []
    for t, (n, off, use_idx, canon) in enumerate(((1, 0, True, True), (255, 0, True, True), (256, 1, True, False), (257, 0, True, True), (13, 0, True, False), (3, 1, False, True),
                                                   (4, 0, False, False), (0, 0, False, True))):
        idx = [rng.randrange(4 - off) for _ in range(n)] if use_idx else None
        tasks.append(dict(n=n, off=off, idx=idx, canonical=canon, out_first=3 + 17 * t, scalars=fix_scalars(cb, n, 61 + t)))
    return dict(name=op, nc=4, tasks=tasks)
