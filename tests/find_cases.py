"""Key sets of the find-trackers tests (tests/test_find_trackers_cpu.py checks them against the g++ twin of find_plan.hpp,
tests/test_gpu_find_trackers.py sends them through the device): plain Python integers, no library under test involved.

The table path of cpx_whisk_find_trackers writes a reduced key k < r in 32 signed radix-256 digits of the WHOLE scalar,
k = sum d_w 256^w with d_w in [-128, 127] (a byte of 0x80 or more borrows from the next window), and reads entry (w, |d_w|) of the
tracker's table, negated for d_w < 0.  The coverage set is built from chosen digits so that every (window, magnitude, sign) a reduced
scalar can ask for occurs in it."""
R_ = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
WINDOWS = 32
ONES = sum(1 << (8 * w) for w in range(WINDOWS - 1))   # 0x01 in each of the lower 31 bytes


def signed_digits(k):
    """the 32 signed radix-256 digits of 0 <= k < r"""
    assert 0 <= k < R_
    out, carry = [], 0
    for w in range(WINDOWS):
        x = ((k >> (8 * w)) & 0xff) + carry
        carry = 1 if x >= 128 else 0
        out.append(x - 256 if x >= 128 else x)
    assert carry == 0 and sum(d << (8 * w) for w, d in enumerate(out)) == k      # no carry leaves the top window: k < r < 2^255
    return out


def top_digit_max():
    """the largest top digit of a reduced scalar: the top byte of r - 1 plus the carry its lower bytes send up"""
    return signed_digits(R_ - 1)[-1]


def attainable_picks():
    """every (window, magnitude, negated) some k < r asks for.  Lower windows: a digit is byte + carry - (256 if that is >= 128), so it
    takes every value in [-128, 127] — magnitude 128 only negated; the top window: 0 .. top byte of r - 1 plus a carry, never negative.
    Each pick is shown attainable by a witness below r."""
    picks = set()
    for w in range(WINDOWS - 1):
        for d in list(range(1, 128)) + list(range(-128, 0)):
            k = d << (8 * w) if d > 0 else (1 << (8 * (w + 1))) + (d << (8 * w))     # a negative digit borrows from the byte above
            assert k < R_ and signed_digits(k)[w] == d
            picks.add((w, abs(d), int(d < 0)))
    for t in range(1, top_digit_max() + 1):
        k = t << (8 * (WINDOWS - 1))
        if k >= R_:
            k = R_ - 1
        assert signed_digits(k)[-1] == t
        picks.add((WINDOWS - 1, t, 0))
    assert all(signed_digits(k)[-1] <= top_digit_max() for k in (R_ - 1, R_ - 2, (R_ - 1) // 2))
    return picks


def picks_of(keys):
    return {(w, abs(d), int(d < 0)) for k in keys for w, d in enumerate(signed_digits(k % R_)) if d}


def coverage_keys():
    """255 keys whose lower 31 digits all equal d, for every d in [-128, 127] but 0, their top digits running through 1 .. 0x73; and
    r - 1, the one source of the top digit 0x74"""
    out = []
    for i, d in enumerate(list(range(1, 128)) + list(range(-128, 0))):
        top = 1 + i % 0x73
        k = (top << (8 * (WINDOWS - 1))) + d * ONES
        assert 0 < k < R_ and signed_digits(k) == [d] * (WINDOWS - 1) + [top]
        out.append(k)
    out.append(R_ - 1)
    return out


def edge_keys():
    """0, 1, r - 1, 2^b and 2^b - 1 around byte boundaries, and the 0x80 / 0x7f byte patterns at the two ends of the carries"""
    out = [0, 1, R_ - 1, R_ - 2, 2]
    for b in (7, 8, 9, 15, 16, 17, 127, 128, 129, 247, 248, 249, 254):
        out += [1 << b, (1 << b) - 1]
    p80, p7f = int.from_bytes(b"\x80" * 31, "little"), int.from_bytes(b"\x7f" * 31, "little")
    out += [p80, p7f, p80 + (0x72 << 248), p7f + (0x73 << 248), int.from_bytes(b"\x80" * 32, "little") % R_, int.from_bytes(b"\x7f" * 32, "little") % R_]
    seen, uniq = set(), []
    for k in out:
        if k not in seen:
            seen.add(k)
            uniq.append(k)
    assert all(0 <= k < R_ for k in uniq)
    return uniq


def to_bytes(keys):
    """canonical little-endian, 32 bytes each"""
    return b"".join((k % R_).to_bytes(32, "little") for k in keys)
