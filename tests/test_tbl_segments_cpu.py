"""CPU checks of the window -> (copy, weight class) map of the shifted tables (curdleproofs_amd/csrc/recode.hpp tbl_window) together
with the recoding it sits on (glv.hpp: the endomorphism split and the signed radix-256 digits of a half), compiled with the host
compiler by tests/host_emul/tbl_segments_emul.cpp.  For the one-segment layout (16 shifted copies per half) and the two-segment one
(8 copies, windows 8..15 in the class of weight 2^64), against Python integers:

    sum_w d_w 2^(8 copy(w)) 2^(8 real class(w))  ==  the half,   copy(w) < real,   +-(+-|t| + q z^2)  ==  k  (mod r).

A half of sixteen 0x80 bytes is outside the domain of the recoding (glv.hpp: a half is at most 0x7f7f...7f, the halves of a split
scalar have a top byte of at most 0x56; the carry of the top window would leave the 128 bits), so the "carry through every window"
case keeps the top byte below that bound: fifteen 0x80 bytes under a top byte of 0x00 and of 0x56 — every window carries into the
next one, the top one included as a receiver.

The partial-slot layout of the bucket-list waves (recode.hpp tbw_parts, tbw_part_slot) is checked for every window grouping, both
table layouts and the wave without shifted copies: the contract between the wave that writes a slot and the planner that tells the
finalisation how many of a task's partials, the first ones, carry the weight 2^64."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_emul", "tbl_segments_emul.cpp")
LIB = os.path.join(HERE, "host_emul", "_tbl_segments.so")
CSRC = os.path.join(HERE, "..", "curdleproofs_amd", "csrc")
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
Z2 = 0xd201000000010000 ** 2   # z^2: (z^2) P = -phi(P) on the order-r subgroup (glv.hpp)


@pytest.fixture(scope="module")
def emul():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("recode.hpp", "glv.hpp", "mont32.hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _words(x, n):
    return (ctypes.c_uint32 * n)(*[(x >> (32 * i)) & 0xffffffff for i in range(n)])


def _int(words):
    return sum(int(w) << (32 * i) for i, w in enumerate(words))


def _check_half(value, real, first, digits, copy, cls):
    assert all(-128 <= d <= 127 for d in digits)
    off = real if first >= 16 else 0           # the endomorphism images follow the `real` shifted copies
    assert all(off <= c < off + real for c in copy), "a window reads a copy the table does not hold"
    assert all(c < 2 * real for c in copy)
    assert all(k == (w % 16) // real for w, k in zip(range(first, first + 16), cls))
    assert sum(d << (8 * (c - off) + 8 * real * k) for d, c, k in zip(digits, copy, cls)) == value
    if real == 8:
        assert all(c - off < 8 for c in copy)
        for k in (0, 1):   # the windows of a class carry weight 1 among themselves: each copy once per class
            assert sorted(c - off for c, kk in zip(copy, cls) if kk == k) == list(range(8))


def _half(L, v, real, first=0):
    d, c, k = (ctypes.c_int32 * 16)(), (ctypes.c_uint32 * 16)(), (ctypes.c_uint32 * 16)()
    L.emul_half_windows(_words(v, 4), real, first, d, c, k)
    _check_half(v, real, first, list(d), list(c), list(k))
    return list(d)


def _scalar(L, kv, real):
    t, q, neg = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 2)()
    d, c, k = (ctypes.c_int32 * 32)(), (ctypes.c_uint32 * 32)(), (ctypes.c_uint32 * 32)()
    L.emul_scalar_windows(_words(kv, 8), real, t, q, neg, d, c, k)
    tv, qv = _int(t), _int(q)
    _check_half(tv, real, 0, list(d)[:16], list(c)[:16], list(k)[:16])
    _check_half(qv, real, 16, list(d)[16:], list(c)[16:], list(k)[16:])
    signed = (-tv if neg[1] else tv) + qv * Z2
    assert (-signed if neg[0] else signed) % R == kv % R, "t + q z^2 does not recombine to the scalar"


@pytest.mark.parametrize("real", [16, 8], ids=["one_segment", "two_segments"])
def test_edge_scalars(emul, real):
    for kv in (0, 1, R - 1):
        _scalar(emul, kv, real)


@pytest.mark.parametrize("real", [16, 8], ids=["one_segment", "two_segments"])
def test_halves_with_a_carry_through_every_window_and_with_none(emul, real):
    for first in (0, 16):
        no_carry = int.from_bytes(b"\x7f" * 16, "little")
        assert _half(emul, no_carry, real, first) == [127] * 16
        for top in (0x00, 0x56):
            carries = int.from_bytes(b"\x80" * 15 + bytes([top]), "little")
            d = _half(emul, carries, real, first)
            assert d[0] == -128 and d[1:15] == [-127] * 14 and d[15] == top + 1
        # window 7 carries into window 8: across the boundary of the two weight classes
        across = (0x80 << 56) | (0x05 << 64)
        d = _half(emul, across, real, first)
        assert d[7] == -128 and d[8] == 6 and all(x == 0 for i, x in enumerate(d) if i not in (7, 8))
        across_run = int.from_bytes(b"\x01" * 7 + b"\xff" + b"\x7f" + b"\x00" * 7, "little")   # ... and the carry lands on a digit that is full
        d = _half(emul, across_run, real, first)
        assert d[7] == -1 and d[8] == -128 and d[9] == 1


@pytest.mark.parametrize("real", [16, 8], ids=["one_segment", "two_segments"])
def test_random_scalars(emul, real):
    rnd = random.Random(20240)
    for _ in range(1000):
        _scalar(emul, rnd.randrange(R), real)


def _tbw_shapes():
    """(wpw, segs, waves per task, sets per wave, windows summed by set `s` of wave `wv`)"""
    for segs in (1, 2):
        for wpw in (2, 4, 8, 16, 32):
            both = segs == 2 and wpw >= 16   # a wave of both weight classes: four sets, set // 2 the class (bit 3 of the window)
            def windows(wv, s, wpw=wpw, both=both):
                return [w for w in range(wv * wpw, (wv + 1) * wpw) if not both or (w >> 3) & 1 == s >> 1]
            yield wpw, segs, 32 // wpw, 4 if both else 2, windows
    yield 2, 1, 16, 2, lambda wv, s: [wv, 16 + wv]   # one window of each half per wave, no shifted copies (k_msm_tblw<2, true>)


@pytest.mark.parametrize("slices", [1, 2, 4])
def test_partial_slots_of_the_bucket_waves(emul, slices):
    for wpw, segs, waves, nsets, windows in _tbw_shapes():
        parts = emul.emul_tbw_parts(wpw, segs)
        assert parts == waves * nsets
        slot = {(wv, sl, s): emul.emul_tbw_part_slot(wpw, segs, waves, slices, wv, sl, s) for wv in range(waves) for sl in range(slices) for s in range(nsets)}
        # (a) a bijection onto the task's range of partial slots
        assert sorted(slot.values()) == list(range(slices * parts)), (wpw, segs)
        cls_of = []   # tbl_window(w, 8).cls of the 32 windows
        for first in (0, 16):
            d, copy, c = (ctypes.c_int32 * 16)(), (ctypes.c_uint32 * 16)(), (ctypes.c_uint32 * 16)()
            emul.emul_half_windows(_words(0, 4), 8, first, d, copy, c)
            cls_of += list(c)
        hi = 0
        for (wv, sl, s), v in slot.items():
            ws = windows(wv, s)
            assert ws and set(ws) <= set(range(32))
            if segs == 1:
                assert v == 2 * (wv * slices + sl) + s                                # (b) waves in order
            else:
                cls = {cls_of[w] for w in ws}
                assert len(cls) == 1, "a set sums windows of both weight classes"
                assert (v < slices * parts // 2) == (cls == {1}), (wpw, wv, sl, s)    # (c) class 1 first
                hi += cls == {1}
            # (d) the lower and the upper magnitudes of one (wave, class) side by side
            assert s % 2 == 0 or (v % 2 == 1 and slot[(wv, sl, s - 1)] == v - 1)
        assert hi == slices * emul.emul_tbw_parts_hi(wpw, segs)                       # what the planner records as tbl_hi
