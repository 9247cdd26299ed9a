"""Model and harness of tests/device/msm_check.hip for tests/test_msm_check_cpu.py and tests/test_gpu_msm_waves.py.

The model is plain Python integers and restates the documented contracts, never the code under test: the scalar split of glv.hpp
(tests/scalar_cases.py py_split), the signed radix-256 digits of glv_biased_bytes, the round rule of tbw_sort's comment, the set layout
and the partial slots of the comments of msm_body.hpp and recode.hpp.  Group elements appear only in the expectation of a bucket: the
sum of the tagged table entries (tests/msm_cases.py) the model puts there, added up by the oracle (orc.g1_msm, naive, unit scalars: a
negative entry enters as the negated point).  The device's entries are compared as group elements (orc.g1_eq_jac), not as limbs: the
order of the LDS atomics inside a list is free."""
import os
import struct

import numpy as np

from tests import check_harness as ch
from tests import msm_cases as mc
from tests.check_harness import list_operations, read_records   # noqa: F401
from tests.msm_cases import NONE, NEG, CANONICAL, TBW_CAP, ROUND_PTS, ROUND_PTS_PERWIN, FIX_CHUNK, POOL
from tests.scalar_cases import P, R, py_split

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "device", "msm_check.hip")
GROUPS = ("sort", "tblw", "pair", "fix", "reduce", "finalize")
TABLE = {"pool": "pool"}
TABLE.update({op: "sort" for op in mc.SORTS})
TABLE.update({op: ("pair" if op == "pair" else "tblw") for op in mc.FORMS})
TABLE.update({op: "fix" for op in mc.FIX_FORMS})
TABLE.update({"reduce/wave": "reduce", "reduce/sets": "reduce", "finalize/wave": "finalize", "finalize/ranges": "finalize", "tail/wave": "finalize", "tail/lanes": "finalize"})
AFF, JAC = 96, 144
ONE_WORD = {op: (1, 1) for op in TABLE}      # the record format of tests/check_harness.py with one word per row


def words(v, n):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def scalar_words(k, canonical):
    return words(k if canonical else k * (1 << 256) % R, 8)


def bytes_words(b):
    return list(struct.unpack("<%dI" % (len(b) // 4), b))


# ---------------------------------------------------------------- the pool of unrelated points and sums over it

class Pool:
    def __init__(self, orc, seed=4242, pts=None):
        self.orc = orc
        self.pts = orc.rng(seed).g1_affine(POOL) if pts is None else pts
        self.one = orc.fr_from_u64(1)
        self.ident = orc.g1_msm(b"", b"")
        self._neg = {}

    def point(self, ref):
        """the 96 bytes of a reference: a pool index, NEG for the negated point, NONE for the identity"""
        if ref == NONE:
            return bytes(AFF)
        i = ref & (NEG - 1)
        a = self.pts[AFF * i:AFF * (i + 1)]
        if not ref & NEG:
            return a
        if i not in self._neg:      # -y in Montgomery form is p - y
            self._neg[i] = a[:48] + (P - int.from_bytes(a[48:], "little")).to_bytes(48, "little")
        return self._neg[i]

    def sum(self, refs):
        refs = [r for r in refs if r != NONE]
        if not refs:
            return self.ident
        return self.orc.g1_msm(b"".join(self.point(r) for r in refs), self.one * len(refs), naive=True)

    def weighted(self, refs, weights):
        pairs = [(r, w) for r, w in zip(refs, weights) if r != NONE]
        if not pairs:
            return self.ident
        sc = b"".join(self.orc.fr_from_canonical_bytes((w % R).to_bytes(32, "little")) for _, w in pairs)
        return self.orc.g1_msm(b"".join(self.point(r) for r, _ in pairs), sc, naive=True)

    def record(self):
        return ("pool", bytes_words(self.pts))


# ---------------------------------------------------------------- scalars -> digits (glv.hpp's documented contract)

def biased_digits(v):
    """glv_biased_bytes: byte w of v + 0x80..80 is d_w + 128, d_w in [-128, 127], sum d_w 256^w = v"""
    b = v + int("80" * 16, 16)
    d = [((b >> (8 * w)) & 0xff) - 128 for w in range(16)]
    assert b < 1 << 128 and sum(x << (8 * w) for w, x in enumerate(d)) == v
    return d


def split_digits(k):
    """(the 32 window digits: 0..15 of |t|, 16..31 of q; the sign the |t| half carries; the sign the q half carries) with
    k = +-(+-|t| + q z^2): the sum of sign * digit * 256^(w mod 16) * (z^2 for w >= 16) is k mod r"""
    t, q, nk, nt = py_split(k)
    return biased_digits(t) + biased_digits(q), nk ^ nt, nk


def digit_words(k):
    """the 9 words k_to_table_endo leaves per scalar (kernels.h TblTask::digits): 32 biased digit bytes and the two half signs"""
    d, lo, hi = split_digits(k)
    return [sum((d[4 * x + b] + 128) << (8 * b) for b in range(4)) for x in range(8)] + [lo | (hi << 1)]


def wave_windows(wpw, perwin, wv):
    """the windows of wave wv in entry order j = 0, 1, ...: wpw consecutive ones, or (PERWIN) window wv of either half"""
    return [wv, 16 + wv] if perwin else list(range(wv * wpw, wv * wpw + wpw))


def n_waves(wpw, perwin):
    return 16 if perwin else 32 // wpw


def point_entries(sd, windows, nbins):
    """the entries (j, bin, negative) of one scalar in one wave; nbins = 256: class x magnitude, the class of window w is (w mod 16) div 8"""
    d, lo, hi = sd
    out = []
    for j, w in enumerate(windows):
        if d[w]:
            b = abs(d[w]) - 1 + (128 * ((w % 16) // 8) if nbins == 256 else 0)
            out.append((j, b, (1 if d[w] < 0 else 0) ^ (lo if w < 16 else hi)))
    return out


def sort_rounds(sds, windows, perwin, nbins, first, ntot):
    """The rounds of one wave over the points [first, ntot) by the rule in tbw_sort's comment: 64-point slabs while
    end - next + 64 <= ROUND_PTS and the entries stay within TBW_CAP, the first slab always.  Per round: next, end, cnt[], cur[] (the
    exclusive prefix sums in bin order plus the sizes: where the cursors stand after the scatter), order[] (bins ascending by size, then
    index), lists[bin] = sorted entry codes ((point - next) << shift | j << 1 | sign), ents = (point, j, bin, negative)."""
    limit, esh = (ROUND_PTS_PERWIN, 2) if perwin else (ROUND_PTS, 6)
    ents = {i: point_entries(sds[i], windows, nbins) for i in range(first, ntot)}
    rounds, nxt = [], first
    while True:
        end, total = nxt, 0
        while end < ntot and end - nxt + 64 <= limit:
            top = min(end + 64, ntot)
            ct = sum(len(ents[i]) for i in range(end, top))
            if total and total + ct > TBW_CAP:
                break
            total, end = total + ct, top
        cnt, lists, flat = [0] * nbins, [[] for _ in range(nbins)], []
        for i in range(nxt, end):
            for j, b, neg in ents[i]:
                cnt[b] += 1
                lists[b].append(((i - nxt) << esh) | (j << 1) | neg)
                flat.append((i, j, b, neg))
        cur, o = [], 0
        for b in range(nbins):
            o += cnt[b]
            cur.append(o)
        rounds.append(dict(next=nxt, end=end, total=total, cnt=cnt, cur=cur, order=sorted(range(nbins), key=lambda b: (cnt[b], b)), lists=[sorted(l) for l in lists],
                           ents=flat, by=("ntot" if end == ntot else "cap" if end - nxt + 64 <= limit else "round_pts")))
        nxt = end
        if nxt >= ntot:
            return rounds


# ---------------------------------------------------------------- the bucket-list waves: buckets and partial slots

def part_slot(wpw, segs, waves, slices, wv, slice_, set_):
    """recode.hpp's comment on tbw_part_slot: a wave leaves the lower and the upper magnitudes at adjacent slots 2k, 2k + 1, k counting
    (wave, slice) in order.  Two-segment tables: the slots of weight class 1 come first, then those of class 0; a wave of up to 8 windows
    lies inside one class (blocks of 8 windows alternate 0, 1, 0, 1), a wave of 16 or 32 windows leaves four sets, set div 2 the class."""
    if segs != 2:
        return 2 * (wv * slices + slice_) + set_
    if wpw >= 16:
        cls, k, per_cls = set_ >> 1, wv, 2 * waves * slices
    else:
        per8 = 8 // wpw
        blk = wv // per8
        cls, k, per_cls = blk & 1, (blk >> 1) * per8 + wv % per8, waves * slices
    return (0 if cls else per_cls) + 2 * (k * slices + slice_) + (set_ & 1)


def table_copy(w, perwin, j, segs):
    """the copy window w reads: its own (32-copy tables), w mod 8 of its half (two-segment tables: 8 + 8 copies), or (PERWIN: P and
    -phi(P)) the half"""
    if perwin:
        return j
    return (w % 16) % 8 + (8 if w >= 16 else 0) if segs == 2 else w


def address(tk, g, copy):
    """(table, element, copy) of point g of a task in table copy `copy` (kernels.h: entry (c, i) at base + c * copy_stride + i; seg[0] then seg[1])"""
    n0 = tk["segs"][0]["n"]
    s, i = (0, g) if g < n0 else (1, g - n0)
    sg = tk["segs"][s]
    return sg["table"], sg["off"] + copy * sg["stride"] + (sg["idx"][i] if sg["idx"] is not None else i), copy


def body_model(case):
    """Per wave (in launch order): dict(task, wv, slice, slots[set], buckets[set][pos] = [(ref, table, element, (point, copy))], rounds).  Bucket b lives at
    position b % 64 of set b / 64, class-major for the two-class waves, + 2 for the second task of a pair."""
    kind, wpw, perwin, segs = mc.FORMS[case["form"]]
    pair, both = kind == "pair", segs == 2 and wpw >= 16
    nbins, nsets, waves, slices = (256 if both else 128), (4 if pair or both else 2), n_waves(wpw, perwin), case["slices"]
    out = []
    step = 2 if pair else 1
    for t in range(0, len(case["tasks"]), step):
        tk = case["tasks"][t]
        sds = [split_digits(k) for k in tk["scalars"]]
        nall = len(sds)
        per = ((nall + slices - 1) // slices + 63) & ~63
        for wv in range(waves):
            wins = wave_windows(wpw, perwin, wv)
            for sl in range(slices):
                first = min(nall, sl * per)
                ntot = min(nall, first + per)
                rounds = sort_rounds(sds, wins, perwin, nbins, first, ntot)
                buckets = [[[] for _ in range(64)] for _ in range(nsets)]
                for rd in rounds:
                    for g, j, b, neg in rd["ents"]:
                        for h in range(step):
                            tb, el, cp = address(case["tasks"][t + h], g, table_copy(wins[j], perwin, j, segs))
                            ref = case["tables"][tb][el]
                            buckets[2 * h + (b >> 6)][b & 63].append((ref if ref == NONE else ref ^ (NEG if neg else 0), tb, el, (g, cp)))
                slots = [(case["tasks"][t + 1]["pad"] if pair and s >= 2 else tk["pad"]) + part_slot(wpw, segs, waves, slices, wv, sl, s & 1 if pair else s) for s in range(nsets)]
                out.append(dict(task=t, wv=wv, slice=sl, first=first, ntot=ntot, slots=slots, buckets=buckets, rounds=rounds))
    return out


def tblw_record(case):
    w = [case["slices"], len(case["tasks"]), len(case["tables"])]
    for tb in case["tables"]:
        w += [len(tb)] + tb
    for tk in case["tasks"]:
        w += [CANONICAL if tk["canonical"] else 0, tk["pad"], 1 if tk["digits"] else 0, len(tk["scalars"])]
        for s in tk["segs"]:
            w += [s["table"], s["off"], s["stride"], s["n"], len(s["idx"]) if s["idx"] is not None else 0]
        for k in tk["scalars"]:
            w += scalar_words(k, tk["canonical"])
        if tk["digits"]:
            for k in tk["scalars"]:
                w += digit_words(k)
        for s in tk["segs"]:
            w += s["idx"] or []
    return (case["form"], w)


def _entry(a, o):
    """(144 bytes, flag) of the raw-set entry at word o"""
    return a[o:o + 36].tobytes(), int(a[o + 36])


def check_sets(pool, what, a, o, expected, where, fmt="table %d element %d (point %d, copy %d)"):
    """a[o:]: 37 words per entry; expected: list of lists of (reference, address...), one per entry; where(e) names entry e.  Returns the
    number compared."""
    for e, refs in enumerate(expected):
        got, flag = _entry(a, o + 37 * e)
        adds = ", ".join(("-" if x[0] != NONE and x[0] & NEG else "+") + fmt % (x[1:3] + tuple(x[3])) for x in refs[:16]) + (" and %d more" % (len(refs) - 16) if len(refs) > 16 else "") or "nothing"
        assert not flag & 2, "%s %s: never written (still the poison; every bin of a round is written, whoever walks it); the model puts there: %s" % (what, where(e), adds)
        live = [x[0] for x in refs if x[0] != NONE]
        if not live:    # a bucket no digit reaches (or identity entries only) is the identity in every form, not merely a point that decodes to it
            assert flag & 1, "%s %s: not the identity; the model puts there: %s" % (what, where(e), adds)
            continue
        assert pool.orc.g1_eq_jac(got, pool.sum(live)), "%s %s: not the sum of the table entries %s" % (what, where(e), adds)
    return len(expected)


def check_tblw(pool, case, out):
    """one output record against the model; returns the number of buckets compared (waves x sets x 64, asserted)"""
    a = out.reshape(-1)
    model = body_model(case)
    what = "%s case %s (slices %d)" % (case["form"], case["name"], case["slices"])
    waves, nsets = int(a[0]), int(a[1])
    assert waves == len(model) and nsets == len(model[0]["slots"]), what
    assert a[2] == 0 and a[3] == 0, "%s: %d / %d words of the guard sets before / after the raw sets were overwritten" % (what, a[2], a[3])
    assert a[4] == 0, "%s: raw_slot was written outside the waves' own entries" % what
    slots = a[5:5 + waves * nsets].tolist()
    o, n = 5 + waves * nsets, 0
    assert len(a) == o + 37 * 64 * waves * nsets, what
    for wi, m in enumerate(model):
        who = "%s task %d wave %d (windows %s) slice %d [%d, %d), %d rounds" % (what, m["task"], m["wv"], wave_windows(*mc.FORMS[case["form"]][1:3], m["wv"]), m["slice"], m["first"], m["ntot"],
                                                                                len(m["rounds"]))
        assert slots[wi * nsets:(wi + 1) * nsets] == m["slots"], "%s: raw_slot %s, the model says %s" % (who, slots[wi * nsets:(wi + 1) * nsets], m["slots"])
        for s in range(nsets):
            binof = (lambda e: 64 * s + e) if nsets == 2 or case["form"] != "pair" else (lambda e: 64 * (s & 1) + e)
            n += check_sets(pool, who, a, o + 37 * 64 * (wi * nsets + s), m["buckets"][s], lambda e: "set %d position %d (bucket of magnitude %d, entries per round %s)" % (
                s, e, 64 * (s & 1) + e + 1, [rd["cnt"][binof(e)] for rd in m["rounds"]]))
    assert n == waves * nsets * 64
    return n


# ---------------------------------------------------------------- sort records

def sort_record(op, scalars, first, ntot, canonical):
    w = [CANONICAL if canonical else 0, 1 if mc.SORTS[op][3] else 0, first, ntot, len(scalars)]
    for k in scalars:
        w += scalar_words(k, canonical)
    if mc.SORTS[op][3]:
        for k in scalars:
            w += digit_words(k)
    return (op, w)


def check_sort(op, name, scalars, first, ntot, out):
    """exactly, except for the order inside a list; returns the number of rounds compared"""
    wpw, perwin, nbins, _ = mc.SORTS[op]
    a = out.reshape(-1).tolist()
    sds = [split_digits(k) for k in scalars]
    assert a[0] == n_waves(wpw, perwin), op
    o, n = 2, 0
    for wv in range(a[0]):
        rounds = sort_rounds(sds, wave_windows(wpw, perwin, wv), perwin, nbins, first, ntot)
        who = "%s case %s wave %d (windows %s), points [%d, %d)" % (op, name, wv, wave_windows(wpw, perwin, wv), first, ntot)
        assert a[o] == len(rounds), "%s: %d rounds, the model says %d (ending at %s)" % (who, a[o], len(rounds), [r["end"] for r in rounds])
        o += 1
        for ri, rd in enumerate(rounds):
            end, total = a[o], a[o + 1]
            cnt, cur, order = a[o + 2:o + 2 + nbins], a[o + 2 + nbins:o + 2 + 2 * nbins], a[o + 2 + 2 * nbins:o + 2 + 3 * nbins]
            lst = a[o + 2 + 3 * nbins:o + 2 + 3 * nbins + total]
            o += 2 + 3 * nbins + total
            rw = "%s round %d from point %d" % (who, ri, rd["next"])
            assert end == rd["end"], "%s: ends at %d, the model says %d (limit: %s)" % (rw, end, rd["end"], rd["by"])
            assert cnt == rd["cnt"], "%s: cnt[] differs first at bin %d" % (rw, next(b for b in range(nbins) if cnt[b] != rd["cnt"][b]))
            assert total == rd["total"], rw
            assert cur == rd["cur"], "%s: the cursors differ first at bin %d" % (rw, next(b for b in range(nbins) if cur[b] != rd["cur"][b]))
            assert order == rd["order"], "%s: order[] differs first at rank %d: bin %d (size %d), the model says bin %d (size %d)" % (
                (rw,) + next((r, order[r], cnt[order[r]] if order[r] < nbins else -1, rd["order"][r], cnt[rd["order"][r]]) for r in range(nbins) if order[r] != rd["order"][r]))
            for b in range(nbins):
                got = sorted(lst[rd["cur"][b] - cnt[b]:rd["cur"][b]])
                assert got == rd["lists"][b], "%s: list of bin %d holds %s, the model says %s" % (rw, b, [hex(x) for x in got[:12]], [hex(x) for x in rd["lists"][b][:12]])
            n += 1
    assert o == len(a), op
    return n


# ---------------------------------------------------------------- fixed-base waves

def fix_digits(k, cb):
    """signed radix-2^cb digits in [-2^(cb-1), 2^(cb-1) - 1] (recode.hpp's contract; the device's recoding is checked digit for digit by
    tests/test_gpu_scalar.py)"""
    d, half = [], 1 << (cb - 1)
    for _ in range(-(-256 // cb)):
        x = k & ((1 << cb) - 1)
        x = x - (1 << cb) if x >= half else x
        d.append(x)
        k = (k - x) >> cb
    assert k == 0
    return d


def fix_model(op, case):
    """the table rows the case's digits reach, each with a tag of its own, and per wave the 64 lane sums: lane l = window l div LPW of the
    wave, point slice l mod LPW (every FIX_CHUNK points of a task start the slices anew)"""
    cb, wpw = mc.FIX_FORMS[op]
    W = -(-256 // cb)
    lpw, rows, waves, tg = 64 // wpw, {}, [], mc.Tags()
    for t, tk in enumerate(case["tasks"]):
        ds = [fix_digits(k, cb) for k in tk["scalars"]]
        for wg in range(W // wpw):
            lanes = [[] for _ in range(64)]
            for l in range(wpw * lpw):
                w, sl = wg * wpw + l // lpw, l % lpw
                for g in range(tk["n"]):
                    if (g % FIX_CHUNK) % lpw == sl and ds[g][w]:
                        key = (w, abs(ds[g][w]) - 1, tk["off"] + (tk["idx"][g] if tk["idx"] is not None else g))
                        if key not in rows:
                            rows[key] = tg.fresh(1)[0]
                        lanes[l].append((rows[key] ^ (NEG if ds[g][w] < 0 else 0), w, key[1], (key[2], g)))
            waves.append(dict(task=t, wg=wg, slot=tk["out_first"] + wg, lanes=lanes))
    return rows, waves


def fix_record(op, case):
    rows, _ = fix_model(op, case)
    w = [case["nc"], len(case["tasks"]), len(rows)]
    for (win, m, col), tag in sorted(rows.items()):
        w += [win, m, col, tag]
    for tk in case["tasks"]:
        w += [CANONICAL if tk["canonical"] else 0, tk["off"], tk["n"], tk["out_first"], len(tk["idx"]) if tk["idx"] is not None else 0]
        for k in tk["scalars"]:
            w += scalar_words(k, tk["canonical"])
        w += tk["idx"] or []
    return (op, w)


def check_fix(pool, op, case, out):
    a = out.reshape(-1)
    _, waves = fix_model(op, case)
    assert int(a[0]) == len(waves), op
    assert a[1] == 0 and a[2] == 0, "%s: %d / %d words of the guard sets before / after the raw sets were overwritten" % (op, a[1], a[2])
    assert a[3] == 0, "%s: raw_slot was written outside the waves' own entries" % op
    slots, o, n = a[4:4 + len(waves)].tolist(), 4 + len(waves), 0
    assert len(a) == o + 37 * 64 * len(waves), op
    for wi, m in enumerate(waves):
        who = "%s task %d (n = %d) wave %d" % (op, m["task"], case["tasks"][m["task"]]["n"], m["wg"])
        assert slots[wi] == m["slot"], "%s: raw_slot %d, the model says out_first + wave = %d" % (who, slots[wi], m["slot"])
        n += check_sets(pool, who, a, o + 37 * 64 * wi, m["lanes"], lambda e: "lane %d (window %d, point slice %d)" % (e, m["wg"] * mc.FIX_FORMS[op][1] + e // (64 // mc.FIX_FORMS[op][1]), e % (64 // mc.FIX_FORMS[op][1])),
                        fmt="window %d row %d (|digit| - 1) column %d (point %d)")
    assert n == 64 * len(waves)
    return n


# ---------------------------------------------------------------- the library's reducers on crafted sets

def reduce_sets(rng):
    """the crafted sets of one kind, as lists of 64 references"""
    p, q = 17, 23
    sets = [("all identity", [NONE] * 64)]
    sets += [("one entry at %d" % l, [p + l if i == l else NONE for i in range(64)]) for l in range(64)]
    sets += [("all 64 the same point", [p] * 64), ("P, -P alternating", [p | (NEG if i & 1 else 0) for i in range(64)])]
    sets += [("P at %d, -P at %d" % (l, l + 1), [q if i == l else q | NEG if i == l + 1 else NONE for i in range(64)]) for l in range(63)]
    sets += [("random %d" % j, [rng.randrange(POOL) | (NEG if rng.randrange(2) else 0) if rng.randrange(8) else NONE for _ in range(64)]) for j in range(4)]
    sets += [("random, repeated points %d" % j, [100 + rng.randrange(3) | (NEG if rng.randrange(2) else 0) for _ in range(64)]) for j in range(2)]
    return sets


def reduce_case():
    """(nplain, nweighted, sets): sets = (name, kind, slot, refs); the plain sets first, then lower / upper alternating; the slots reversed"""
    import random
    sets = reduce_sets(random.Random(70))
    assert len(sets) % 2 == 0
    rows = [(n, "plain", r) for n, r in sets]
    for n, r in sets:
        rows += [(n, "lower", r), (n, "upper", r)]
    return len(sets), 2 * len(sets), [(n, k, len(rows) - 1 - i, r) for i, (n, k, r) in enumerate(rows)]


def reduce_record(op, case):
    nplain, nweighted, sets = case
    w = [nplain, nweighted]
    for _, _, slot, refs in sets:
        w += [slot] + refs
    return (op, w)


def check_reduce(pool, op, case, out):
    a = out.reshape(-1)
    _, _, sets = case
    assert int(a[0]) == len(sets) and len(a) == 1 + 37 * len(sets), op
    for si, (name, kind, slot, refs) in enumerate(sets):
        got, flag = _entry(a, 1 + 37 * slot)
        who = "%s set %d (%s, %s) -> partial slot %d" % (op, si, kind, name, slot)
        assert not flag & 2, "%s: never written" % who
        weights = [1 if kind == "plain" else l + 1 if kind == "lower" else 64 + l + 1 for l in range(64)]
        assert pool.orc.g1_eq_jac(got, pool.weighted(refs, weights)), "%s: not the sum of weight x entry (weights %d..%d)" % (who, weights[0], weights[-1])
    return len(sets)


# ---------------------------------------------------------------- finalisation and Horner tail

def jac_of(aff):
    """an affine point as a Jacobian one with Z = 1 (Montgomery form: 2^384 mod p)"""
    return aff + ((1 << 384) % P).to_bytes(48, "little") if any(aff) else IDENT


IDENT = ((1 << 384) % P).to_bytes(48, "little") * 2 + bytes(48)


def jac_neg(j):
    return j[:48] + ((P - int.from_bytes(j[48:96], "little")) % P).to_bytes(48, "little") + j[96:]


def finalize_case(pool, n):
    """n requests cycling through: the (c, hi) pairs (0, 0), (1, 0), (1, 1), (5, 0), (5, 2), (5, 5) on distinct partial sums with Z != 1, on equal
    ones (doublings in the additions), on opposite ones (the running sum passes through the identity, the request ends as the identity) and on
    identities; then up to three affine addends with holes, one of them equal to the running sum.  dst_index and comp_index scatter."""
    orc = pool.orc
    J = [orc.g1_add_jac(jac_of(pool.point(2 * i)), jac_of(pool.point(2 * i + 1))) for i in range(8)]       # Z != 1
    shapes = [(0, 0), (1, 0), (1, 1), (5, 0), (5, 2), (5, 5)]
    fills = {"distinct": lambda c: J[:c], "equal": lambda c: [J[5]] * c, "opposite": lambda c: ([J[6], jac_neg(J[6])] * 3)[:c] if c != 5 else [J[6], jac_neg(J[6]), IDENT, J[7], jac_neg(J[7])],
             "identity": lambda c: [IDENT] * c, "mixed": lambda c: ([J[1], IDENT, J[1], jac_neg(J[2]), J[3]])[:c]}
    templates = [(s, f, add) for f in fills for s in shapes for add in (None,)] + [(s, "distinct", add) for s in shapes for add in ("one", "equal", "three")]
    parts, reqs, sources = [], [], [pool.point(900 + i) for i in range(4)]
    for g in range(n):
        (c, hi), fill, add = templates[g % len(templates)]
        mine = fills[fill](c)
        scal = b"".join(orc.fr_from_canonical_bytes(((1 << 64) if j < hi else 1).to_bytes(32, "little")) for j in range(c))
        want = orc.g1_msm_jac(b"".join(mine), scal) if c else IDENT
        addends = [NONE, NONE, NONE]
        if add == "one":
            addends = [NONE, n + g % 4, NONE]
        elif add == "three":
            addends = [n + (g + 1) % 4, n + g % 4, n + g % 4]            # the same point twice: P + P in the mixed addition
        elif add == "equal":                                              # an addend equal to the running sum
            sources.append(orc.g1_to_affine(want))
            addends = [NONE, NONE, n + len(sources) - 1]
        reqs.append(dict(first=len(parts) if c else 0, c=c, hi=hi, fill=fill, add=add, addends=addends, want=want))
        parts += mine
    for rq in reqs:
        w = rq["want"]
        for x in rq["addends"]:
            if x != NONE:
                w = orc.g1_add_jac(w, jac_of(sources[x - n]))
        rq["aff"] = orc.g1_to_affine(w)
        rq["comp"] = orc.g1_compress(rq["aff"])
    dst = [(7 * g + 3) % n for g in range(n)] if n % 7 else list(range(n))
    ci = [n - 1 - g + 2 for g in range(n)]
    return dict(n=n, parts=parts, reqs=reqs, sources=sources, dst=dst, ci=ci, ncomp=n + 2)


def finalize_record(op, fc):
    n = fc["n"]
    w = [n, len(fc["parts"]), n + len(fc["sources"]), fc["ncomp"], 1, 1, 1]
    w += bytes_words(b"".join(fc["parts"])) + bytes_words(bytes(AFF) * n + b"".join(fc["sources"]))
    w += [rq["first"] for rq in fc["reqs"]] + [rq["c"] | (rq["hi"] << 16) for rq in fc["reqs"]] + fc["dst"] + fc["ci"]
    for rq in fc["reqs"]:
        w += rq["addends"]
    return (op, w)


def check_finalize(op, fc, out):
    a = out.reshape(-1)
    n, naff = fc["n"], fc["n"] + len(fc["sources"])
    assert len(a) == 24 * naff + 12 * fc["ncomp"], op
    for g, rq in enumerate(fc["reqs"]):
        who = "%s request %d of %d: %d partial sums from %d, the first %d of weight 2^64, %s, addends %s" % (op, g, n, rq["c"], rq["first"], rq["hi"], rq["fill"], rq["add"])
        assert a[24 * fc["dst"][g]:24 * fc["dst"][g] + 24].tobytes() == rq["aff"], "%s: the point at dst_index %d is not the oracle's" % (who, fc["dst"][g])
        o = 24 * naff + 12 * fc["ci"][g]
        assert a[o:o + 12].tobytes() == rq["comp"], "%s: the 48 bytes at comp_index %d are not the oracle's" % (who, fc["ci"][g])
    assert a[24 * n:24 * naff].tobytes() == b"".join(fc["sources"]), "%s: the addend sources were overwritten" % op
    free = sorted(set(range(fc["ncomp"])) - set(fc["ci"]))
    assert all(a[24 * naff + 12 * i:24 * naff + 12 * i + 12].tobytes() == b"\xa5" * 48 for i in free), "%s: compressed bytes outside comp_index" % op
    return n


def tail_case(pool, nout, group, shift, dup, extra):
    orc = pool.orc
    J = [orc.g1_add_jac(jac_of(pool.point(300 + 2 * i)), jac_of(pool.point(301 + 2 * i))) for i in range(12)]
    import random
    rng = random.Random(80 + nout + dup)
    ins, exs, want = [], [], []
    for t in range(nout):
        mine = [rng.choice(J + [IDENT]) for _ in range(group * dup)]
        if dup > 1:
            mine[0:2] = [J[0], J[0]]                         # equal inputs of one window: a doubling in the tree
            if group > 1:
                mine[dup:dup + 2] = [J[1], jac_neg(J[1])]    # opposite ones: the window sum is the identity
        if t == 1:
            mine = [IDENT] * (group * dup)
        ex = [rng.choice(J) for _ in range(extra)]
        sc = [1 << (shift * (i // dup)) for i in range(group * dup)] + [1] * extra
        want.append(orc.g1_msm_jac(b"".join(mine + ex), b"".join(orc.fr_from_canonical_bytes((s % R).to_bytes(32, "little")) for s in sc)))
        ins += mine
        exs += ex
    return dict(nout=nout, group=group, shift=shift, dup=dup, extra=extra, ins=ins, exs=exs, want=want)


def tail_record(op, tc):
    return (op, [tc["nout"], tc["group"], tc["shift"], tc["dup"], tc["extra"]] + bytes_words(b"".join(tc["ins"])) + bytes_words(b"".join(tc["exs"])))


def check_tail(pool, op, tc, out):
    a = out.reshape(-1)
    assert len(a) == 36 * tc["nout"], op
    for t in range(tc["nout"]):
        assert pool.orc.g1_eq_jac(a[36 * t:36 * t + 36].tobytes(), tc["want"][t]), "%s output %d (group %d, shift %d, dup %d, %d extra): not sum_j 2^(shift j) (inputs of window j) + extras" % (
            op, t, tc["group"], tc["shift"], tc["dup"], tc["extra"])
    return tc["nout"]


# ---------------------------------------------------------------- running

def pack_records(records):
    """records: list of (operation, words): a record of one word per row"""
    return ch.pack_records(ONE_WORD, [(name, np.asarray(w, dtype=np.int64).reshape(-1, 1)) for name, w in records])


def run(exe, records, work_dir, tag, timeout=120):
    """one process: every record through `exe`; the outputs in order, one per record.  A nonzero exit fails at once; nothing is retried."""
    res = read_records(ch.run_file(exe, pack_records(records), work_dir, tag, timeout, "%d records" % len(records)))
    assert [n for n, _ in res] == [n for n, _ in records]
    return [a for _, a in res]
