"""The scalars, half-size values and inversion inputs of the scalar-side checks, defined once: tests/scalar_check_lib.py turns them
into the rows of tests/device/scalar_check.hip and tests/test_gpu_scalar_mul_edges.py runs the edge scalars through the kernels.  Everything is a Python integer; nothing here looks at the code under test.
py_split is the split of glv.hpp restated on integers (one division), used to name what a scalar exercises, never as an expectation."""
import random

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
Z = 0xd201000000010000
Z2 = Z * Z                       # N of glv.hpp: phi acts as multiplication by -z^2
H2 = Z2 // 2
HALF_BOUND = (1 << 127) - (1 << 119)
BIASED_MAX = int("7f" * 16, 16)   # glv_biased_bytes: the largest value 16 digits in [-128, 127] add up to
FIX_CB = (8, 16, 19)


def fix_windows(cb):
    return -(-256 // cb)


def py_split(k):
    """(|t|, q, neg_k, neg_t) with k = +-(+-|t| + q z^2) mod r, k' = min(k, r - k) = q z^2 + t, |t| <= z^2 / 2"""
    nk = 1 if k > (R - 1) // 2 else 0
    kk = R - k if nk else k
    q, rem = divmod(kk + H2, Z2)
    t = rem - H2
    return abs(t), q, nk, 1 if t < 0 else 0


def naf(v):
    """the non-adjacent form of v >= 0, digit i at index i"""
    out = []
    while v:
        d = 0
        if v & 1:
            d = 2 - (v & 3)
            v -= d
        out.append(d)
        v >>= 1
    return out


Q_MAX = ((R - 1) // 2 + H2) // Z2          # the largest q a scalar < r reaches

# the directed scalars, by name: the sign turns of k and t, the multiples of z^2 around them, the word boundaries of the split
EDGE_SCALARS = {
    "0": 0, "1": 1, "2": 2, "r-1": R - 1, "r-2": R - 2, "(r-1)/2": (R - 1) // 2, "(r+1)/2": (R + 1) // 2,
    "z2": Z2, "z2-1": Z2 - 1, "z2+1": Z2 + 1, "z2/2": H2, "z2/2-1": H2 - 1, "z2/2+1": H2 + 1, "r-z2": R - Z2,
    "(r-1)/2-z2/2": (R - 1) // 2 - H2, "2^127": 1 << 127, "2^128-1": (1 << 128) - 1, "2^254": 1 << 254, "2^255 mod r": (1 << 255) % R,
    "(2^127-1) z2": ((1 << 127) - 1) * Z2 % R, "qmax z2": Q_MAX * Z2,
    "r - z2/2": R - H2, "r - z2/2 - 1": R - H2 - 1, "r - 1 - z2": R - 1 - Z2, "r - qmax z2": R - Q_MAX * Z2,
}


def _pattern(byte, n=31, top=0x73):
    """n low bytes of `byte` under the top byte `top`: below r for top = 0x73 and a byte below 0xed, or a smaller top"""
    return int.from_bytes(bytes([byte]) * n + bytes(32 - n - 1) + bytes([top if n == 31 else 0]), "little")


def pattern_scalars():
    out = []
    for b in (0x80, 0x7f, 0x88, 0x99, 0x55, 0xaa, 0x33, 0xcc, 0xff, 0x77):
        out += [_pattern(b, 31, 0x73 if b < 0xed else 0x72), _pattern(b, 31, 0), int.from_bytes(bytes([b]) * 32, "little") % R, int.from_bytes(bytes([b]) * 16, "little")]
    return out


def threshold_scalars(cb):
    """every chunk at (2^(cb-1)) and one below its carry threshold, alone, under a run of all-ones chunks (the carry runs on), and all
    chunks together alternating; only values below r"""
    half, full, w = 1 << (cb - 1), 1 << cb, fix_windows(cb)
    out = []
    for j in range(w):
        for c in (half, half - 1):
            out.append(c << (cb * j))
            above = cb * (j + 1)
            if above < 254:
                out.append((c << (cb * j)) | (((1 << 254) - 1) >> above << above))   # all ones above up to bit 253: the carry runs on
    out.append(sum((half - (j & 1)) << (cb * j) for j in range(255 // cb)))
    out.append(sum((half - 1 + (j & 1)) << (cb * j) for j in range(255 // cb)))
    out.append(sum(half << (cb * j) for j in range(255 // cb)))
    return [v for v in out if v < R]


def scalar_cases(n_random=3200, seed=20260):
    """canonical scalars (< r): the edges, the patterns, every chunk threshold, 2^b and 2^b - 1 for every b < 255, seeded random values"""
    rng = random.Random(seed)
    out = list(EDGE_SCALARS.values()) + pattern_scalars()
    for cb in FIX_CB:
        out += threshold_scalars(cb)
    for b in range(255):
        out += [1 << b, (1 << b) - 1]
    out += [rng.randrange(R) for _ in range(n_random)]
    out += [rng.randrange(1 << b) for b in range(1, 255, 2)]
    assert all(0 <= v < R for v in out)
    return out


def half_cases(scalars, n_random=1200, seed=20261):
    """values below 2^127 (an endomorphism half): directed bytes and nibbles, the halves of the scalars' own splits, random values"""
    rng = random.Random(seed)
    out = [0, 1, 8, 9, 15, 16, 127, 128, 129, 255, 256, (1 << 127) - 1, HALF_BOUND - 1, H2, H2 + 1, Q_MAX, int("8" * 31, 16), int("9" * 31, 16),
           int("7" + "f" * 31, 16), int("7" + "8" * 31, 16), int("7" + "9" * 31, 16), int("80" * 15, 16), int("7f" * 16, 16), int("7f" + "80" * 15, 16),
           int("55" * 16, 16), int("2a" + "aa" * 15, 16), int("33" * 16, 16), int("77" * 16, 16)]
    out += [1 << b for b in range(127)] + [(1 << b) - 1 for b in range(127)]
    for k in scalars[:1400]:
        t, q, _, _ = py_split(k)
        out += [t, q]
    out += [rng.randrange(1 << 127) for _ in range(n_random)]
    assert all(0 <= v < (1 << 127) for v in out)
    return out


def naf_cases(scalars, halves):
    """recode_naf takes any 8 words: canonical scalars (the plain form of k_smul), halves (the split form) and raw 256-bit values whose
    form has its 257th digit, at bit 256"""
    raw = [(1 << 256) - 1, (1 << 256) - 2, int("aa" * 32, 16), int("55" * 32, 16), int("33" * 32, 16), int("cc" * 32, 16), 3 << 254, (1 << 255) + 1,
           (1 << 255) | (1 << 254) | 1, int("b" * 64, 16), int("ab" * 32, 16), 1 << 255, (1 << 255) - 1, 1 << 128, 3 << 127, (1 << 129) - 1]
    raw += [(3 << (b - 1)) for b in range(1, 256)]                      # 11 at every position: the carry into the digit above
    return raw + scalars[:2600] + halves[:1200]


# ---------------------------------------------------------------- inversions

def divstep_count(a, p):
    """the number of division steps (Bernstein-Yang, delta = -eta starting at eta = -1) until g = 0 from (f, g) = (p, a)"""
    f, g, eta, n = p, a, -1, 0
    while g:
        z = (g & -g).bit_length() - 1
        g >>= z
        eta -= z
        n += z
        if eta < 0:
            eta, f, g = -eta, g, -f
        g = (g + f) >> 1
        eta -= 1
        n += 1
    return n


def batch_count(a, p):
    """batches of 30 division steps words_inv_divsteps runs for the input a: it stops after the first batch that leaves g = 0"""
    return max(1, -(-divstep_count(a, p) // 30))


def batch_search(p, seed, n_random, n_fib, keep=24):
    """the seeded search for inputs that take many batches: random values and ratios F_(n+1) / F_n mod p of Fibonacci-like sequences
    from random starts; returns the `keep` inputs with the highest counts, highest first"""
    rng = random.Random(seed)
    cand = [rng.randrange(1, p) for _ in range(n_random)]
    for _ in range(n_fib // 64):
        a, b = rng.randrange(1, 1 << 16), rng.randrange(1, 1 << 16)
        for _ in range(64):
            a, b = b, (a + b) % p
            if a % p:
                cand.append(b * pow(a, -1, p) % p)
    cand = [c for c in cand if c]
    return sorted(set(cand), key=lambda c: (-batch_count(c, p), c))[:keep]


# batch_search(P, 381, 20000, 4096, keep=8) and batch_search(R, 255, 20000, 4096, keep=8) (seed, random values, Fibonacci-like ratios):
# the inputs with the most batches found, 28 each mod p and 19 each mod r
HIGH_COUNT_P = [
    0x3297de9d4b80bdda70895646ca8758513fd5360f1ec15338f9705acf7bd5034d7faefa8a5a80eb9c9b5d5ad6d784c,
    0x92ce44cc09661c3b0286e645b3dd43f7884321f1e12243d3e92307d29f7b7c95bce965a73996981eadf79fd02d49d,
    0x38dfc962c941ffdc6f903ce2665949b2ebccf2412113a33df5f728dee1141d587275c3d44e22722668d35435c1935a,
    0x40243313b0fab035a3e2c59916534ad787fc44edea31c38817bea7bc79d58aab8d66f127662182eea658674a4f7ac4,
    0x67333ef517d79d17d1bd220177e276fde10bb2adb3e4c6a3af02dba2c2e03504cbb1fefa5dc3c700e38e5cee6d1de4,
    0x7d7cce951cf2665fe519c204fbcd4a0b957392d0ea2e9b4df78c87fdfa60220fdf25771a6e2122a62af2dfe7359518,
    0x803842d5a5902166d19504083c673092fd9946fb1d320fcf936ba1e1b84ec4ec89b3e81163a914a4ad1158d56c06a9,
    0x8d1cd882dff4793b904e5f47214d2bf48e8c25572556777e8c49fb866a15c03255fce2fda83f5bf14e57299b3396cc,
]
HIGH_COUNT_R = [
    0x31cd52c7b562fb966c5bb9a586b99d61a76609510c4f76b7510e867ac4c67,
    0x2f74cb452e83dbfad9714748f8e44b8b16f3fd66a5313d92b5190976e3a67b,
    0x3366e6e1ad3e97bea42780f496bafdebb51e74ad9b25011302b2ded5ac4d36,
    0x3ae13d55d8b42f4206ed927c329b3ec93a9cf8e817c64fd819f111973b0c15,
    0x3bd1c0e99cd73ff0909f7fb97012589e09fd15e5d732ffad87fb0d570c2e9e,
    0x48fcbac15cc86e46323955d9e59b13bd696b99d86ac510a239cbe21cb850ba,
    0x550a62df3b21188f55f4eb680180cf05cb52db03c96c94280e00d2db507fa8,
    0x6383049ab3169157ef0965bd73e210e473ed3e49d57b21ec0d9a9fec1108da,
]


def inversion_inputs(p, bits, high, n_random=1100, seed=30):
    rng = random.Random(seed + bits)
    out = [0, 1, 2, 3, 4, 5, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 30, (1 << 30) - 1, 0x3fffffff << 30, (1 << 60) + 1, (1 << 60) - 1, 1 << 60,
           0x3fffffff << 60, (1 << 90) + (1 << 30), p >> 1, p >> 30, p - (1 << 30), p - (1 << 30) + 1]
    out += [1 << b for b in range(bits)] + [(1 << b) - 1 for b in range(1, bits + 1) if (1 << b) - 1 < p]
    out += list(high)
    out += [rng.randrange(1, p) for _ in range(n_random)] + [rng.randrange(1, 1 << b) for b in range(1, bits, 3)]
    assert all(0 <= v < p for v in out)
    return out


def divsteps_rows(seed=31):
    """(eta, f0, g0) of one batch: f0 odd below 2^30; eta over the range the inversions reach and beyond, g0 = 0, odd, even, powers of two"""
    rng = random.Random(seed)
    top = (1 << 30) - 1
    fs = [1, 3, top, top - 2, 0x2aaaaaab, 0x15555555, (1 << 29) + 1, P & top, R & top]
    gs = [0, 1, 2, 3, top, top - 1, 1 << 29, 1 << 15, (1 << 29) + 1, 0x2aaaaaaa, 0x15555555, 0x3ffffffe]
    out = [(eta, f, g) for eta in (-1, 0, 1, -2, 7, -8, 29, -30, 30, -31, 31, 383, -383, 766, -766) for f in fs for g in gs]
    for eta in range(-800, 801):
        out.append((eta, rng.randrange(1 << 30) | 1, rng.randrange(1 << 30)))
    for _ in range(1000):
        out.append((rng.randrange(-40, 41), rng.randrange(1 << 30) | 1, rng.randrange(1 << 30) >> rng.randrange(30) << rng.randrange(20) & top))
    return out
