"""Scalar sets of the generator-table tests (tests/test_generator_mul_cpu.py checks them against the g++ twin of gen_table.hpp,
tests/test_gpu_generator_mul.py sends them through the device): plain Python integers, no library under test involved.

A scalar is split as k = sk (t + q z^2) mod r with |t| <= z^2 / 2 (curdleproofs_amd/csrc/glv.hpp); both halves are written in 16 signed
radix-256 digits, the lower 15 in [-128, 127], the top one in [0, 0x56].  The coverage set is built from chosen halves so that every
(half, window, digit magnitude, sign of the pick) the table can be asked for occurs in it."""
R_ = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
Z = 0xd201000000010000
Z2 = Z * Z
HALF_R = (R_ - 1) // 2
WINDOWS = 16


def signed_digits(v):
    """the 16 signed radix-256 digits of 0 <= v < 2^127: byte w of v + 0x80..80, minus 128 (glv.hpp glv_biased_bytes)"""
    assert 0 <= v < 1 << 127
    b = v + int.from_bytes(b"\x80" * 16, "little")
    assert b < 1 << 128
    d = [((b >> (8 * w)) & 0xff) - 128 for w in range(WINDOWS)]
    assert sum(x << (8 * w) for w, x in enumerate(d)) == v
    return d


def split(k):
    """(neg_k, neg_t, |t|, q) with k = (-1)^neg_k ((-1)^neg_t |t| + q z^2) mod r, k' = min(k, r - k), q = round(k' / z^2)"""
    k %= R_
    neg_k = k > HALF_R
    kp = R_ - k if neg_k else k
    q = (kp + Z2 // 2) // Z2
    t = kp - q * Z2
    assert abs(t) <= Z2 // 2
    return int(neg_k), int(t < 0), abs(t), q


def from_halves(t, q, neg_k):
    """the scalar whose split is (neg_k, t < 0, |t|, q); t signed"""
    kp = t + q * Z2
    assert 0 < kp <= HALF_R and abs(t) < Z2 // 2 and q >= 0
    k = R_ - kp if neg_k else kp
    assert split(k) == (int(neg_k), int(t < 0), abs(t), q)
    return k


def top_digit_max():
    """the largest top digit either half can have"""
    t_max = Z2 // 2
    q_max = (HALF_R + Z2 // 2) // Z2
    return max(signed_digits(t_max)[-1], signed_digits(q_max)[-1])


def _value(lower_digit, top):
    return sum(lower_digit << (8 * w) for w in range(WINDOWS - 1)) + (top << (8 * (WINDOWS - 1)))


def coverage_scalars():
    """every lower window gets every digit in [-128, 127] \\ {0}, in both halves, under every sign combination (neg_k, neg_t); the top
    window gets every digit 1 .. 0x56 the same way"""
    top_max = top_digit_max()
    out = []
    for m in range(1, 129):
        top = 1 + (m - 1) % (top_max - 1)          # 1 .. top_max - 1: any lower digits fit below z^2 / 2
        for d in (m, -m):
            if d == 128:
                continue
            v = _value(d, top)
            assert signed_digits(v)[:-1] == [d] * (WINDOWS - 1) and signed_digits(v)[-1] == top
            for neg_t in (0, 1):
                for neg_k in (0, 1):
                    out.append(from_halves(-v if neg_t else v, v, neg_k))
    v = _value(1, top_max)                          # the largest top digit: small lower digits keep the halves in range
    assert signed_digits(v)[-1] == top_max
    for neg_t in (0, 1):
        for neg_k in (0, 1):
            out.append(from_halves(-v if neg_t else v, v, neg_k))
    return out


def all_picks():
    """every (half, window, magnitude, negated) the table can be asked for"""
    top_max = top_digit_max()
    return {(h, w, m, s) for h in (0, 1) for w in range(WINDOWS) for m in range(1, (top_max if w == WINDOWS - 1 else 128) + 1) for s in (0, 1)}


def edge_scalars():
    lo80 = int.from_bytes(b"\x80" * 15, "little")   # halves whose lower 15 bytes are 0x80 (digit -128, then -127 under the carry) ...
    lo7f = int.from_bytes(b"\x7f" * 15, "little")   # ... and 0x7f (digit +127): the two ends of the digit range
    return [0, 1, 2, R_ - 1, R_ - 2,
            Z2, Z2 - 1, Z2 + 1, Z2 // 2, (R_ + 1) // 2, (R_ - 1) // 2,
            (1 << 128) - 1, 1 << 127,
            int.from_bytes(b"\x80" * 32, "little") % R_, int.from_bytes(b"\x7f" * 32, "little") % R_,
            from_halves(lo80, lo80, 0), from_halves(-lo80, lo80, 1), from_halves(lo7f, lo7f, 0), from_halves(-lo7f, lo7f, 1),
            127, 128, 255, 256]


def to_bytes(scalars):
    return b"".join((k % R_).to_bytes(32, "little") for k in scalars)
