"""Pure-Python model of ark-ec 0.4 `G1Projective::rand` on the reference's StdRng (tests/stdrng_ref.py, unchanged), for the tests of
rng_fp_accept / rng_g1_candidate (curdleproofs_amd/csrc/rng.hpp), g1_28_point_from_x / g1_28_clear_cofactor (g1_28.hpp) and cpx_rng_g1.
Restated from the algorithm, in Python integers, not from the product headers:

    loop:  x = six next_u64, least significant first, masked to 381 bits; rejected (nothing else drawn) when >= p.  The limbs ARE the
           Montgomery form of x (R = 2^384).  An accepted x is followed by one u32 whose top bit is `greatest`.  If x^3 + 4 is a square, the
           draw is [h](x, y), y the larger of (y, p - y) iff greatest, h the full cofactor; otherwise the loop goes on.

tests/test_rng_g1_check_cpu.py pins it against the oracle's `g1_affine` (oracle/stdrng.h), which the reference's known-answer tests pin.
The walk records where every candidate started and what became of it; tests/rng_g1_cases.py searches those records for its cases."""
from tests.stdrng_ref import R as R_ORDER

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
H = 0x396c8c005555e1568c00aaab0000aaab           # |E(Fp)| / r
N_CURVE = H * R_ORDER
RMONT = (1 << 384) % P
RINV = pow(RMONT, -1, P)
MASK381 = (1 << 381) - 1
assert H == 3 * 11 ** 2 * 10177 ** 2 * 859267 ** 2 * 52437899 ** 2 and P % 4 == 3

REJECTED, NO_ROOT, POINT = "rejected", "no root", "point"


def fp_accept(value):
    """the 384-bit integer of twelve stream words -> (masked value, accepted)"""
    v = value & MASK381
    return v, v < P


# ---- the curve y^2 = x^3 + 4 over Fp, affine, None = the identity ----
def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def mul(k, a):
    """[k] a for any integer k >= 0 and any point of E(Fp)"""
    r = None
    while k:
        if k & 1:
            r = add(r, a)
        a = add(a, a)
        k >>= 1
    return r


def on_curve(a):
    return a is None or (a[1] * a[1] - a[0] ** 3 - 4) % P == 0


def point_from_x(x, greatest):
    """x: the field element (not its Montgomery limbs); None where x^3 + 4 is not a square"""
    rhs = (x * x * x + 4) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return None
    if (y > P - y) != bool(greatest):
        y = P - y
    return x, y % P


def clear_cofactor(a):
    return mul(H, a)


def to_wire(a):
    """96 bytes: Montgomery limbs of x and y, little-endian; the identity is all zero"""
    if a is None:
        return bytes(96)
    return (a[0] * RMONT % P).to_bytes(48, "little") + (a[1] * RMONT % P).to_bytes(48, "little")


def from_wire(b):
    if bytes(b) == bytes(96):
        return None
    return int.from_bytes(b[:48], "little") * RINV % P, int.from_bytes(b[48:96], "little") * RINV % P


def compress(a):
    """the 48-byte encoding (zcash flags: compressed, infinity, larger y)"""
    if a is None:
        return bytes([0xc0]) + bytes(47)
    b = bytearray(a[0].to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if a[1] > P - a[1] else 0)
    return bytes(b)


def mont_words(x):
    """the twelve 32-bit Montgomery limbs of a field element, least significant first"""
    v = x * RMONT % P
    return [(v >> (32 * i)) & 0xffffffff for i in range(12)]


# ---- the token walk ----
class Walk:
    """G1::rand on `rng` (a tests.stdrng_ref.StdRng, advanced): `tokens` lists (word_pos of the candidate, kind, position behind the token)
    for every candidate met, in order"""

    def __init__(self, rng):
        self.rng = rng
        self.tokens = []

    def candidate(self):
        """one accepted candidate: (Montgomery limbs as an integer, greatest, word_pos it started at)"""
        rng = self.rng
        while True:
            at = rng.word_pos
            v = 0
            for i in range(6):
                v |= rng.next_u64() << (64 * i)
            v, ok = fp_accept(v)
            if ok:
                return v, rng.next_u32() >> 31, at
            self.tokens.append((at, REJECTED, rng.word_pos))

    def point_unscaled(self):
        """the point before the cofactor multiplication"""
        while True:
            v, greatest, at = self.candidate()
            pt = point_from_x(v * RINV % P, greatest)
            self.tokens.append((at, POINT if pt else NO_ROOT, self.rng.word_pos))
            if pt:
                return pt

    def g1(self):
        return clear_cofactor(self.point_unscaled())

    def g1_affine(self, n=1):
        """wire bytes of n draws, as the oracle's Rng.g1_affine"""
        return b"".join(to_wire(self.g1()) for _ in range(n))


def g1_affine(rng, n=1):
    return Walk(rng).g1_affine(n)
