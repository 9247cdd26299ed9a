"""The cases of the G1::rand tests, held once: tests/test_rng_g1_check_cpu.py states what they cover and runs the rows through the host twin
of tests/device/rng_g1_check.hip, tests/test_gpu_rng_g1.py runs the same ones through the gfx950 build and through cpx_rng_g1.

Streams are descriptors: ("seed", seed, offset) = StdRng::seed_from_u64(seed) advanced by `offset` words — the oracle can follow those, so
their expected POINTS are the oracle's — and ("state", 40 bytes) for the starts the oracle cannot reach (a high block counter, children of a
split), whose points are the integer model's (tests/stdrng_g1_ref.py); those stay below 200 points over all tests.  POSITIONS and hit
patterns are the model's everywhere.  The cases that need an accident of the stream are found by a search over seeds 0, 1, 2, ... that
stops at the first hit, as tests/rng_cases.edge_cases does."""
import functools
import math
import os
import struct

import numpy as np

from tests import check_harness as ch
from tests import rng_cases as rc
from tests import stdrng_g1_ref as g1
from tests import stdrng_ref as sr
from tests.check_harness import list_operations, read_records   # noqa: F401
from tests.stdrng_ref import StdRng

WINDOW_WORDS = 64 * 16            # the scan window of k_rng_g1_scan (curdleproofs_amd/csrc/rng_g1_plan.hpp): 64 blocks from the block of the next token
SEEDS = (0, 1, 7, (1 << 64) - 1)
SHAPES = ((1, 1), (1, 300), (3, 65), (65, 1), (65, 8))   # (count, n_each) of cpx_rng_g1, as the issue names them
CAPS = (1, 2, 64)                 # option rng_g1_round_cap for the later rounds
EDGE_CAP, EDGE_NEED = 8, 4        # the two round-boundary cases (below)


def default_cap(need):
    ceil_sqrt = math.isqrt(need - 1) + 1 if need else 0
    return 2 * need + 8 * ceil_sqrt + 16


def cap(need, round_cap=0):
    d = default_cap(need)
    return min(d, round_cap) if round_cap else d


def rng_of(desc):
    if desc[0] == "seed":
        return StdRng(sr.key_from_u64(desc[1]), desc[2])
    return StdRng.from_state(desc[1])


def state_of(desc):
    return rng_of(desc).state()


@functools.lru_cache(maxsize=None)
def walk(desc, n):
    """model: the tokens of n draws (no cofactor multiplication: positions and hit patterns only), and the position behind them"""
    w = g1.Walk(rng_of(desc))
    for _ in range(n):
        w.point_unscaled()
    return tuple(w.tokens), w.rng.word_pos


@functools.lru_cache(maxsize=None)
def pool():
    """every seed at every start residue mod 16, one high-counter start, two children of a split"""
    streams = [("seed", s, o) for s in SEEDS for o in range(16)]
    streams.append(("state", StdRng(sr.key_from_u64(2), rc.HIGH_POS).state()))
    parent = StdRng.seed_from_u64(3)
    streams += [("state", parent.split().state()), ("state", parent.split().state())]
    return tuple(streams)


@functools.lru_cache(maxsize=None)
def searched():
    """name -> (descriptor, need, round_cap).
    last / first: the need-th point comes from the LAST candidate round one emits / from the FIRST candidate of round two.  Under the default
    cap that is a 5-sigma accident by design (need = 1: the first root at the 26th candidate, 2^-26 per stream), out of a search's reach, so
    the two cases run under rng_g1_round_cap = EDGE_CAP with need = EDGE_NEED: the same boundary of the same code.
    bool first / straddle: a token of the first 65 draws whose bool word is the first word of the next scan window / whose twelve words
    straddle it (default cap).  rejected2 / noroot4: two rejected candidates in a row / four accepted candidates in a row without a root."""
    found = {}
    seed = 0
    while len(found) < 6:
        desc = ("seed", 1000 + seed, seed % 16)
        tokens, _ = walk(desc, 65)
        kinds = [k for _, k, _ in tokens]
        hits = [k == g1.POINT for k in kinds if k != g1.REJECTED]            # per accepted candidate
        nth = [i for i, h in enumerate(hits) if h]                           # index of the candidate that supplies point j
        if "last" not in found and nth[EDGE_NEED - 1] == EDGE_CAP - 1:
            found["last"] = (desc, EDGE_NEED, EDGE_CAP)
        elif "first" not in found and nth[EDGE_NEED - 1] == EDGE_CAP:
            found["first"] = (desc, EDGE_NEED, EDGE_CAP)
        used = set(at for at, _, _ in tokens)                                 # tokens the 65 draws consume
        ev_at = _edge_tokens(desc, 65)
        for name in ("bool first", "straddle"):
            if name not in found and any(at in used for at in ev_at[name]):
                found[name] = (desc, 65, 0)
        if "rejected2" not in found and any(kinds[i] == kinds[i + 1] == g1.REJECTED for i in range(min(len(kinds), 40) - 1)):
            found["rejected2"] = (desc, 8, 0)
        acc_kinds = [k for k in kinds if k != g1.REJECTED]
        if "noroot4" not in found and any(all(k == g1.NO_ROOT for k in acc_kinds[i:i + 4]) for i in range(min(len(acc_kinds), 30) - 3)):
            found["noroot4"] = (desc, 8, 0)
        seed += 1
    return found


def _edge_tokens(desc, n):
    """word_pos of the tokens that meet a window edge in round one, by kind of accident"""
    tokens, _ = walk(desc, n)               # (the scan goes on behind them; what it meets there is never used)
    want, emitted = cap(n), 0
    out = {"bool first": [], "straddle": []}
    base = tokens[0][0] & ~15
    for at, kind, _ in tokens:
        if emitted == want:
            break
        words = 12 if kind == g1.REJECTED else 13
        if at + words > base + WINDOW_WORDS:
            out["straddle" if at + 12 > base + WINDOW_WORDS else "bool first"].append(at)
            base = at & ~15
        emitted += kind != g1.REJECTED
    return out


def shape_streams(count):
    """the streams of a (count, .) shape: 1 -> seed 0 from the start; 3 -> a seed stream at an odd offset, the high counter, a child;
    65 -> 62 seed streams (every residue), the high counter, both children"""
    p = pool()
    if count == 1:
        return (p[0],)
    if count == 3:
        return (p[16 + 5], p[64], p[65])
    assert count == 65
    return p[:62] + p[64:]


def g1_cases():
    """[(streams, n_each, round_cap)] of cpx_rng_g1 under the default cap (round_cap 0) and the searched ones at their own"""
    out = [(shape_streams(c), n, 0) for c, n in SHAPES]
    for name, (desc, need, rcap) in sorted(searched().items()):
        out.append(((desc,), need, rcap))
    return out


_EXPECTED = {}


def expected(orc, desc, n):
    """(affine bytes, compressed bytes, state after, the next Fr::rand) of n draws from the stream"""
    key = (desc, n)
    if key in _EXPECTED:
        return _EXPECTED[key]
    _, pos = walk(desc, n)
    after = StdRng(rng_of(desc).key, pos)
    state = after.state()
    nxt = after.fr(1)
    if desc[0] == "seed":
        o = orc.rng(desc[1])
        for _ in range(desc[2]):
            o.u32()
        aff = o.g1_affine(n)
        assert o.fr(1) == nxt, "the model's position behind %d draws is not the oracle's" % n
        comp = b"".join(g1.compress(g1.from_wire(aff[96 * i: 96 * i + 96])) for i in range(n))
    else:
        w = g1.Walk(rng_of(desc))
        pts = [w.g1() for _ in range(n)]
        aff = b"".join(g1.to_wire(p) for p in pts)
        comp = b"".join(g1.compress(p) for p in pts)
    _EXPECTED[key] = (aff, comp, state, nxt)
    return _EXPECTED[key]


def model_points_needed():
    """how many points the integer model multiplies by the cofactor over all cpx_rng_g1 cases (the issue's bound: 200)"""
    return sum(n for streams, n, _ in g1_cases() for d in streams if d[0] == "state")


# ---------------------------------------------------------------- rows of tests/device/rng_g1_check.hip
TABLE = {"fp_accept": (12, 13), "g1_candidate": (10, 15), "point_from_x": (13, 25), "clear_cofactor": (24, 24)}
P = g1.P
FP_EDGES = (P - 1, P, P + 1, 0, (1 << 381) - 1, (P - 1) | (1 << 381), (P - 1) | (7 << 381), 5 | (1 << 383), (1 << 384) - 1, P | (1 << 382), P - (1 << 32), P + (1 << 32),
            P - 1 - 0xaaaa, P + 0x5554, (P >> 32 << 32), P ^ (1 << 352))


def words(v, n):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def wire_words(pt):
    return list(struct.unpack("<24I", g1.to_wire(pt)))


@functools.lru_cache(maxsize=None)
def torsion_points():
    """name -> point for the clear_cofactor rows: crafted from model points Q of E(Fp) (not in the subgroup) as (N / q^2) Q with N = h r"""
    w = g1.Walk(StdRng.seed_from_u64(11))
    out = {"identity": None, "(0, 2)": (0, 2), "(0, p - 2)": (0, P - 2)}
    qs = [w.point_unscaled() for _ in range(6)]
    for q in (11, 10177):
        for Q in qs:
            # (q^2 divides h and the q-part of E(Fp) is Z_q x Z_q — E(Fp) = Z_(m/3) x Z_(m r), m = |z - 1| — so (N / q) Q is the identity
            # for every Q; (N / q^2) Q has order q unless Q has no q-part)
            assert g1.mul(g1.N_CURVE // q, Q) is None
            t = g1.mul(g1.N_CURVE // (q * q), Q)
            if t is not None:
                assert g1.mul(q, t) is None and g1.on_curve(t)
                out["order %d" % q] = t
                break
    out["order dividing h"] = g1.mul(sr.R, qs[0])
    assert out["order dividing h"] is not None and g1.mul(g1.H, out["order dividing h"]) is None
    for i, Q in enumerate(qs[:3]):
        out["generic %d" % i] = Q
        out["subgroup %d" % i] = g1.clear_cofactor(Q)
    assert g1.mul(3, (0, 2)) is None
    return out


@functools.lru_cache(maxsize=None)
def check_records():
    """[(operation, rows)] for rng_g1_check"""
    streams = list(pool()) + [d for d, _, _ in searched().values()]
    st = [rc.state_words(state_of(d)) for d in streams]
    first = [[r.word(r.word_pos + i) for i in range(12)] for r in map(rng_of, streams)]
    # x rows: zero with both bools, a non-residue and a residue with both bools, the first candidates of a few streams
    nonres = next(x for x in range(1, 50) if g1.point_from_x(x, 0) is None)
    res = next(x for x in range(1, 50) if g1.point_from_x(x, 0) is not None)
    xs = [(words(0, 12), 0), (words(0, 12), 1), (g1.mont_words(nonres), 0), (g1.mont_words(nonres), 1), (g1.mont_words(res), 0), (g1.mont_words(res), 1)]
    for d in streams[::5]:
        w = g1.Walk(rng_of(d))
        for _ in range(3):
            v, gr, _ = w.candidate()
            xs += [(words(v, 12), gr), (words(v, 12), 1 - gr)]
    rec = [("fp_accept", [words(v, 12) for v in FP_EDGES] + first),
           ("g1_candidate", st),
           ("point_from_x", [x + [b] for x, b in xs]),
           ("clear_cofactor", [wire_words(p) for _, p in sorted(torsion_points().items())])]
    assert [n for n, _ in rec] == list(TABLE)
    return tuple((n, tuple(tuple(r) for r in rows)) for n, rows in rec)


def expected_row(name, row):
    row = list(row)
    if name == "fp_accept":
        v, ok = g1.fp_accept(sum(w << (32 * i) for i, w in enumerate(row)))
        return words(v, 12) + [1 if ok else 0]
    if name == "g1_candidate":
        w = g1.Walk(StdRng(row[:8], row[8] | (row[9] << 32)))
        v, gr, _ = w.candidate()
        return words(v, 12) + [gr] + words(w.rng.word_pos, 2)
    if name == "point_from_x":
        xm = sum(w << (32 * i) for i, w in enumerate(row[:12]))
        pt = g1.point_from_x(xm * g1.RINV % P, row[12])
        return [1] + wire_words(pt) if pt else [0] * 25
    if name == "clear_cofactor":
        return wire_words(g1.clear_cofactor(g1.from_wire(struct.pack("<24I", *row))))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def check_expected():
    return tuple((n, np.array([expected_row(n, r) for r in rows], dtype=np.uint32)) for n, rows in check_records())


SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device", "rng_g1_check.hip")


build_host_twin = functools.partial(ch.build_host_twin, SRC, name="rng_g1_check_host")      # (out_dir, extra=(), name=...)


def run_check(exe, records, work_dir, tag, timeout=300):
    return ch.run(exe, TABLE, records, work_dir, tag, timeout)


assert_rows = ch.assert_same
