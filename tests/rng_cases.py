"""The cases of the rng tests, held once: tests/test_rng_check_cpu.py states what they cover and runs them through the host twin of
tests/device/rng_check.hip, tests/test_gpu_rng.py runs the same ones through the gfx950 build, cpx_rng_fr and cpx_rng_shuffle_draws.
Everything is derived from fixed seeds by the Python model (tests/stdrng_ref.py); the few cases that need a particular accident of the
stream (a draw that ends exactly at a window's edge) are found by a search over seeds 0, 1, 2, ... that stops at the first hit."""
import functools
import os
import struct

import numpy as np

from tests import check_harness as ch
from tests import stdrng_ref as sr
from tests.check_harness import list_operations, read_records   # noqa: F401
from tests.stdrng_ref import R, StdRng

WINDOW = 64                       # candidates k_rng_draw tests per window (curdleproofs_amd/csrc/rng.hip)
N_EACH = (1, 63, 64, 65, 200)     # the sizes the issue names
COUNTS = (1, 3, 65)
HIGH_POS = (1 << 36) - 40         # the block counter's high word changes 40 words on
SHUFFLE_ELLS = (28, 124)


def candidates(rng, n_each):
    """Fr::rand n_each times on a clone of rng: the list of (word_pos, accepted) of every candidate, in order"""
    c = rng.clone()
    c.fr(n_each)
    return sorted([(p, True) for p in c.fr_accepts] + [(p, False) for p in c.fr_rejections])


@functools.lru_cache(maxsize=None)
def edge_cases():
    """(state whose n-th draw is candidate 63 of its first window, n), (state whose n-th draw is candidate 64: the first of the next window, n),
    state with three rejected candidates in a row among its first 64"""
    last = first = run3 = None
    seed = 0
    while not (last and first and run3):
        rng = StdRng.seed_from_u64(1000 + seed)
        rng.word_pos = seed % 16                  # (and not only from offset 0)
        c = candidates(rng, 70)
        acc = [a for _, a in c]
        if not last and acc[63]:
            last = (rng.state(), sum(acc[:64]))
        elif not first and acc[64]:
            first = (rng.state(), sum(acc[:65]))
        if not run3 and any(not any(acc[i:i + 3]) for i in range(60)):
            run3 = rng.state()
        seed += 1
    return last, first, run3


@functools.lru_cache(maxsize=None)
def pool():
    """65 distinct states: one start at each of the 16 word offsets, the high-counter start, the three searched ones, children of one parent"""
    base = StdRng.seed_from_u64(1)
    states = [StdRng(base.key, o).state() for o in range(16)]
    states.append(StdRng(sr.key_from_u64(2), HIGH_POS).state())
    last, first, run3 = edge_cases()
    states += [last[0], first[0], run3]
    parent = StdRng.seed_from_u64(3)
    while len(states) < max(COUNTS):
        states.append(parent.split().state())
    assert len(set(states)) == len(states)
    return tuple(states)


@functools.lru_cache(maxsize=None)
def fr_cases():
    """[(n_each, states)]: every size over the whole pool, the two searched sizes with their state first"""
    last, first, _ = edge_cases()
    p = list(pool())
    out = [(n, tuple(p)) for n in N_EACH]
    for st, n in (last, first):
        out.append((n, tuple([st] + [s for s in p if s != st])))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fr_expected(n_each, states):
    """model: (outputs back to back, states after), for the first len(states) streams"""
    outs, after = [], []
    for s in states:
        rng = StdRng.from_state(s)
        outs.append(rng.fr(n_each))
        after.append(rng.state())
    return b"".join(outs), b"".join(after)


@functools.lru_cache(maxsize=None)
def shuffle_states(ell):
    """three streams per ell: seed 0 from the start (the reference's own), and two children of it at odd offsets"""
    parent = StdRng.seed_from_u64(0)
    a, b = parent.split(), parent.split()
    a.word_pos, b.word_pos = 5, 11 + ell
    return (StdRng.seed_from_u64(0).state(), a.state(), b.state())


@functools.lru_cache(maxsize=None)
def shuffle_expected(ell, states):
    """model: per stream (perm, k, blinders, rand, state after k, state at the end)"""
    out = []
    for s in states:
        rng = StdRng.from_state(s)
        perm, k, mb, rand, mid = rng.shuffle_draws(ell)
        out.append((perm, k, mb, rand, mid, rng.state()))
    return tuple(out)


# ---------------------------------------------------------------- rows of tests/device/rng_check.hip
TABLE = {"chacha12_block": (10, 16), "next_u32": (10, 42), "next_u64": (10, 42), "fr_rand": (10, 34), "fr_accept": (8, 9), "range_accept": (2, 3),
         "gen_range": (11, 3), "shuffle": (11, 42), "seed_from_u64": (2, 10), "split": (10, 12), "pos_valid": (2, 1)}
CHK_SHUFFLE = 40


def words(v, n):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def state_words(s):
    return list(struct.unpack("<10I", s))


SEEDS = (0, 1, 2, 0xdeadbeef, (1 << 32) - 1, 1 << 32, (1 << 63) + 12345, (1 << 64) - 1)
FR_EDGES = (0, 1, R - 1, R, R + 1, (1 << 255) - 1, (1 << 255), (1 << 255) + R - 1, (1 << 256) - 1, R - (1 << 32), R + (1 << 32), R ^ (1 << 224), R - (1 << 224),
            (R >> 32 << 32), (R >> 64 << 64) | ((1 << 64) - 1), R | (1 << 255))
RANGES = tuple(range(1, 131)) + (255, 256, 257, 65535, 65536, 1 << 31, (1 << 31) + 1, (1 << 32) - 1)
V_EDGES = (0, 1, 0x7fffffff, 0x80000000, 0xffffffff, 0xaaaaaaab, 0x55555555)


@functools.lru_cache(maxsize=None)
def check_records():
    """[(operation, rows)] for rng_check: every function of rng.hpp"""
    p = [state_words(s) for s in pool()]
    keys = [x[:8] for x in (p[0], p[16], p[20])]
    counters = (0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, HIGH_POS >> 4, (1 << 60) - 1)
    rec = [("chacha12_block", [k + words(c, 2) for k in keys for c in counters]),
           ("next_u32", p), ("next_u64", p), ("fr_rand", p),
           ("fr_accept", [words(v, 8) for v in FR_EDGES] + [x[:8] for x in p]),
           ("range_accept", [[v, r] for r in RANGES for v in V_EDGES + (p[r % len(p)][0], p[r % len(p)][1])]),
           ("gen_range", [x + [r] for x in p[:20] for r in RANGES[::7] + (3, 5, 6, 7)]),
           ("shuffle", [x + [n] for x in p[:24] for n in (0, 1, 2, 3, 28, CHK_SHUFFLE)]),
           ("seed_from_u64", [words(s, 2) for s in SEEDS]),
           ("split", p),
           ("pos_valid", [words(v, 2) for v in (0, 1, sr.POS_LIMIT - 1, sr.POS_LIMIT, sr.POS_LIMIT + 1, (1 << 64) - 1, 1 << 32, HIGH_POS)])]
    assert [n for n, _ in rec] == list(TABLE)
    return tuple((n, tuple(tuple(r) for r in rows)) for n, rows in rec)


def _rng_of(row):
    return StdRng(row[:8], row[8] | (row[9] << 32))


def expected_row(name, row):
    """the model's answer to one row: a list of output words"""
    row = list(row)
    if name == "chacha12_block":
        return sr.chacha12_block(row[:8], row[8] | (row[9] << 32))
    if name == "fr_accept":
        v = sum(w << (32 * i) for i, w in enumerate(row)) & ((1 << 255) - 1)
        return words(v, 8) + [1 if v < R else 0]
    if name == "range_accept":
        v, r = row
        zone = (((r << (32 - r.bit_length())) & 0xffffffff) - 1) & 0xffffffff
        m = v * r
        return [zone, m >> 32, 1 if (m & 0xffffffff) <= zone else 0]
    if name == "seed_from_u64":
        return sr.key_from_u64(row[0] | (row[1] << 32)) + [0, 0]
    if name == "pos_valid":
        return [1 if (row[0] | (row[1] << 32)) < sr.POS_LIMIT else 0]
    rng = _rng_of(row)
    if name == "next_u32":
        out = [rng.next_u32() for _ in range(40)]
    elif name == "next_u64":
        out = []
        for _ in range(20):
            out += words(rng.next_u64(), 2)
    elif name == "fr_rand":
        out = []
        for _ in range(4):
            out += words(rng.fr_int(), 8)
    elif name == "gen_range":
        out = [rng.gen_range(row[10])]
    elif name == "shuffle":
        n = min(row[10], CHK_SHUFFLE)
        out = rng.shuffle(n) + list(range(n, CHK_SHUFFLE))
    elif name == "split":
        out = state_words(rng.split().state())
    else:
        raise KeyError(name)
    return out + words(rng.word_pos, 2)


# ---------------------------------------------------------------- building and running rng_check (tests/check_harness.py)
SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device", "rng_check.hip")
build_host_twin = functools.partial(ch.build_host_twin, SRC, name="rng_check_host")      # (out_dir, extra=(), name=...)


def run_check(exe, records, work_dir, tag, timeout=120):
    return ch.run(exe, TABLE, records, work_dir, tag, timeout)


@functools.lru_cache(maxsize=None)
def check_expected():
    """the model's answers to check_records(), computed once"""
    return tuple((n, np.array([expected_row(n, r) for r in rows], dtype=np.uint32)) for n, rows in check_records())


assert_rows = ch.assert_same
