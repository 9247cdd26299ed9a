"""Operand sets for the field code of curdleproofs_amd/csrc (fp28.hpp, mont32.hpp, g1_28.hpp) on raw limbs, generated from fixed
seeds at test time.  tests/test_f28_redc_karatsuba_cpu.py (g++ on the bodies of the 28-bit-limb product), tests/test_field_check_cpu.py
(the host twin of tests/device/field_check.hip) and tests/test_gpu_field.py (its gfx950 build) draw the same rows from here."""
import random

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
RMOD = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
R392 = 1 << 392
MASK = (1 << 28) - 1
TOP38 = (38 * P) >> 364          # top limb of a value at the largest operand magnitude of the point formulas (38 p)


def limbs(v):
    """normalised limbs of an integer: 0..12 in [0, 2^28), the top limb signed"""
    out = []
    for _ in range(13):
        out.append(v & MASK)
        v >>= 28
    return out + [v]


def value(ls):
    return sum(x << (28 * i) for i, x in enumerate(ls))


def check_montgomery(t, target):
    """t = (target + M p) / 2^392 for an integer M in [0, 2^392), with normalised limbs"""
    assert all(0 <= x <= MASK for x in t[:13])
    num = value(t) * R392 - target
    assert num % P == 0
    assert 0 <= num // P < R392


def rand_val(rng, scale):
    return rng.randrange(-scale * P, scale * P + 1)


def lazy_diff(x, y):
    """f28_sub_lazy: limb-wise difference of two normalised values, no carry pass"""
    return [p - q for p, q in zip(limbs(x), limbs(y))]


def cneg_lazy(x):
    """f28_cneg_lazy of a normalised value"""
    return [-v for v in limbs(x)]


def product_range(rng):
    """a value in the range of a Montgomery product, (-0.81 p, 1.81 p)"""
    return rng.randrange(-81 * P // 100, 181 * P // 100)


# ---------------------------------------------------------------- operands of the 28-bit-limb products (fp28.hpp)
# Each set: squares (one operand per row), products (rows of two operands), differences a b - c d (rows of four).

def random_sets(seed=3920):
    """random operands at 1, 12 and 38 p: one (scale, squares, products, differences) per scale"""
    rng = random.Random(seed)
    for scale in (1, 12, 38):
        ops = [limbs(rand_val(rng, scale)) for _ in range(400)]
        rows2 = [[limbs(rand_val(rng, scale)), limbs(rand_val(rng, scale))] for _ in range(400)]
        rows4 = [[limbs(rand_val(rng, scale)) for _ in range(4)] for _ in range(400)]
        yield scale, ops, rows2, rows4


def extreme_ops():
    """limbs at +-(2^28 - 1), top limb at its largest lazy value for 38 p, in every sign combination, and single-limb spikes on
    either half of the Karatsuba split"""
    pos = [MASK] * 13 + [TOP38]
    neg = [-MASK] * 13 + [-TOP38]
    alt = [MASK if i % 2 else -MASK for i in range(13)] + [TOP38]
    halves = [[MASK] * 7 + [-MASK] * 6 + [-TOP38], [-MASK] * 7 + [MASK] * 6 + [TOP38]]
    ops = [pos, neg, alt, [-x for x in alt]] + halves + [[0] * 14, limbs(P), limbs(P - 1), limbs(1), limbs(R392 % P)]
    for i in range(14):
        s = [0] * 14
        s[i] = TOP38 if i == 13 else MASK
        ops += [s, [-x for x in s]]
    return ops, pos, neg, alt


def extreme_sets(seed=11):
    """extreme_ops() squared, in every pair and in random fours; the largest column sums of f28_mulsub_body (all four operands at
    the extreme of the same sign); and products whose Montgomery digits (m = -a b p^-1 mod 2^392) are 0, all 2^28 - 1, or one half all
    2^28 - 1 and the other 0: dm_i = m_i - m_(7+i) and the substituted m_(k-7) dP_0 of the Karatsuba reduction at both ends of
    their range.  Returns a dict: squares, pairs, fours, same_sign, digit_rows, digit_fours."""
    ops, pos, neg, alt = extreme_ops()
    rng = random.Random(seed)
    out = {"squares": ops, "pairs": [[a, b] for a in ops for b in ops]}
    out["fours"] = [[rng.choice(ops) for _ in range(4)] for _ in range(3000)]
    out["same_sign"] = [[pos, pos, neg, pos], [neg, neg, pos, neg], [pos, neg, neg, neg], [alt, alt, [-x for x in alt], alt]]
    rows = []
    for m in (0, R392 - 1, (1 << 196) - 1, R392 - (1 << 196)):
        target = -m * P % R392
        for _ in range(4):
            while True:   # a random a within 38 p and b = target / a mod 2^392, kept when b is within 38 p as well
                a = rng.randrange(1, 38 * P) | 1
                b = target * pow(a, -1, R392) % R392
                b = b if b < 38 * P else b - R392
                if abs(b) < 38 * P:
                    break
            assert (-(a * b) * pow(P, -1, R392)) % R392 == m
            rows.append([limbs(a), limbs(b)])
    out["digit_rows"] = rows
    out["digit_fours"] = [r + [limbs(0), limbs(0)] for r in rows] + [r + rows[-1 - k] for k, r in enumerate(rows)]
    return out


def lazy_shape_sets(seed=2801, n2=2000, n4=2000):
    """f28_sub_lazy / f28_cneg_lazy results as operands: limbs in (-2^28, 2^28) of either sign, top limb signed"""
    rng = random.Random(seed)
    prod = lambda: product_range(rng)
    ops = []
    for _ in range(300):
        ops += [lazy_diff(prod(), rand_val(rng, 6)), lazy_diff(rand_val(rng, 15), rand_val(rng, 15)), cneg_lazy(prod()),
                cneg_lazy(rand_val(rng, 3))]
    rows2 = [[rng.choice(ops), rng.choice(ops)] for _ in range(n2)]
    rows4 = [[rng.choice(ops) for _ in range(4)] for _ in range(n4)]
    return ops, rows2, rows4


def point_formula_sets(seed=3811):
    """operands shaped as in xyzz28_add_mixed_t, jac28_dbl, xyzz28_dbl and xyzz28_add (g1_28.hpp): products in (-0.81 p, 1.81 p),
    stored coordinates up to 15.4 p, lazy differences of a product and a coordinate, lazily negated y, shifted values"""
    rng = random.Random(seed)
    prod = lambda: product_range(rng)
    coord = lambda m: rng.randrange(-int(m * P), int(m * P))
    rows2, rows4, sq = [], [], []
    for _ in range(300):
        # mixed addition: U2 = X2 ZZ1, S2 = (+-Y2) ZZZ1, P = U2 - X1, R = S2 - Y1 (lazy), PP = P^2, PPP = P PP, Q = X1 PP,
        # X3 = R^2 - PPP - 2 Q, Y3 = R (Q - X3) - Y1 PPP, ZZ3 = ZZ1 PP, ZZZ3 = ZZZ1 PPP
        x2, y2, zz1, zzz1, x1, y1 = prod(), prod(), prod(), prod(), coord(6.3), coord(2.7)
        pp_, rr = lazy_diff(prod(), x1), lazy_diff(prod(), y1)
        pp2, ppp, qq, x3 = prod(), prod(), prod(), coord(6.3)
        rows2 += [[limbs(x2), limbs(zz1)], [cneg_lazy(y2), limbs(zzz1)], [limbs(zz1), limbs(pp2)], [pp_, limbs(pp2)],
                  [limbs(x1), limbs(pp2)], [limbs(zzz1), limbs(ppp)]]
        sq += [pp_, rr]
        rows4 += [[rr, lazy_diff(qq, x3), limbs(y1), limbs(ppp)]]
        # Jacobian doubling (k_table_build): A = X^2, B = Y^2, F = E^2 with E = 3 A; Y3 = E (D - X3) - (8 B) B with D = 4 X B
        x, y = coord(15.4), coord(15.4)
        e, d, x3d, b = 3 * prod(), 4 * prod(), coord(15.4), prod()
        sq += [limbs(x), limbs(y), limbs(e)]
        rows4 += [[limbs(e), lazy_diff(d, x3d), limbs(8 * b), limbs(b)]]
        # XYZZ doubling: V = (2 Y)^2, XX = X^2, M^2 with M = 3 XX
        sq += [limbs(2 * coord(2.7)), limbs(3 * prod())]
        # full XYZZ addition: R = S2 - S1 (lazy, both products), Y3 = R (Q - X3) - S1 PPP
        s1 = prod()
        rows4 += [[lazy_diff(prod(), s1), lazy_diff(prod(), coord(8.1)), limbs(s1), limbs(prod())]]
        rows2 += [[lazy_diff(prod(), s1), lazy_diff(prod(), prod())]]
    return sq, rows2, rows4


def product_operand_sets():
    """every set above as one list each of squares, products and differences (the rows the device build runs)"""
    sq, rows2, rows4 = [], [], []
    for _, a, b, c in random_sets():
        sq, rows2, rows4 = sq + a, rows2 + b, rows4 + c
    e = extreme_sets()
    sq, rows2, rows4 = sq + e["squares"], rows2 + e["pairs"] + e["digit_rows"], rows4 + e["fours"] + e["same_sign"] + e["digit_fours"]
    for a, b, c in (lazy_shape_sets(), point_formula_sets()):
        sq, rows2, rows4 = sq + a, rows2 + b, rows4 + c
    return sq, rows2, rows4


# ---------------------------------------------------------------- linear operations, zero test, conversions, inversions

def linear_operands(seed=2814):
    """normalised values of either sign up to 38 p and the extremes of normalised limbs (0..12 at 2^28 - 1 or 0, the top limb at
    +-TOP38): what f28_add / f28_sub / f28_sub_sub2 / f28_neg / f28_cneg / f28_shl take"""
    rng = random.Random(seed)
    ops = [limbs(v) for v in (0, 1, -1, P, -P, P - 1, P + 1, 2 * P, 38 * P, -38 * P)]
    ops += [[MASK] * 13 + [TOP38], [MASK] * 13 + [-TOP38], [0] * 13 + [TOP38], [0] * 13 + [-TOP38], [MASK] * 13 + [0], [MASK] * 13 + [-1]]
    for i in range(13):
        s = [0] * 14
        s[i] = MASK
        ops += [s, s[:13] + [-1]]
    for scale in (1, 6, 15, 38):
        ops += [limbs(rand_val(rng, scale)) for _ in range(150)]
    return ops


def normalize_operands(seed=2815):
    """what a carry pass meets: limb-wise sums and differences before it.  f28_sub_sub2 reaches |limb| < 2^30 and f28_shl<3>
    2^31 - 8, so limbs go to the int32 extremes that leave the carry into the next limb representable"""
    rng = random.Random(seed)
    big = (1 << 31) - (1 << 4)
    ops = [[big] * 13 + [TOP38], [-big] * 13 + [-TOP38], [big if i % 2 else -big for i in range(13)] + [0], [-1] * 14, [MASK + 1] * 13 + [0],
           [-(MASK + 1)] * 13 + [0]]
    for _ in range(400):
        ops.append([rng.randrange(-big, big + 1) for _ in range(13)] + [rng.randrange(-TOP38, TOP38 + 1)])
        ops.append(lazy_diff(rand_val(rng, 15), rand_val(rng, 15)))
    return ops


def product_is_zero_operands(seed=2816):
    """values a product can take, (-0.81 p, 1.81 p) with normalised limbs (the header: a product cannot reach -p): 0 and p, the
    neighbours of both, 2 p just outside the range as the nearest other multiple a wrong mask would accept, -1 with its negative top
    limb, and random values"""
    rng = random.Random(seed)
    vals = [0, P, 1, P - 1, P + 1, 2 * P, -1, 2, -2, P - 2, P + 2, R392 % P, P - R392 % P]
    for i in range(14):          # one limb of 0 resp. p off by one bit
        for base in (0, P):
            v = base ^ (1 << (28 * i)) if base else base + (1 << (28 * i))
            if -81 * P // 100 < v < 181 * P // 100:
                vals.append(v)
    vals += [product_range(rng) for _ in range(1500)]
    return [limbs(v) for v in vals]


def conversion_operands(seed=2817):
    """lazy values of either sign up to the documented magnitudes: product range for f28_canonical_words, up to 38 p for f28_to_std
    and the inversions (any lazy value: one product brings it into range); canonical words below p for f28_from_std; any 384-bit
    integer for f28_from_words"""
    rng = random.Random(seed)
    edge = [0, 1, P - 1, P, P + 1, -1, R392 % P, (P - 1) // 2, (P + 1) // 2]
    prod = [limbs(v) for v in edge + [-81 * P // 100 + 1, 181 * P // 100 - 1]] + [limbs(product_range(rng)) for _ in range(600)]
    lazy = [limbs(v) for v in edge + [38 * P, -38 * P, 2 * P, -P, -2 * P]] + [[MASK] * 13 + [TOP38], [MASK] * 13 + [-TOP38]]
    for scale in (1, 6, 15, 38):
        lazy += [limbs(rand_val(rng, scale)) for _ in range(150)]
    lazy += [lazy_diff(product_range(rng), rand_val(rng, 6)) for _ in range(100)] + [cneg_lazy(product_range(rng)) for _ in range(100)]
    std = [0, 1, P - 1, P - 2, (1 << 384) % P, (1 << 768) % P, (P - 1) // 2, (P + 1) // 2, (1 << 380), (1 << 380) - 1]
    std += [rng.randrange(P) for _ in range(600)]
    words = [0, 1, (1 << 384) - 1, P, P - 1, (1 << 383), (1 << 364) - 1, 1 << 364] + [((1 << 28) - 1) << (28 * i) for i in range(14)]
    words = [w & ((1 << 384) - 1) for w in words] + [rng.getrandbits(384) for _ in range(400)]
    return {"product": prod, "lazy": lazy, "std": std, "words": words}


def inversion_operands(seed=2818, n=48):
    """a few lazy values (an inversion is ~570 products): edges, either sign, up to 38 p; 0 and p, whose inverse is 0"""
    rng = random.Random(seed)
    vals = [0, P, 1, -1, P - 1, P + 1, 2, R392 % P, 38 * P - 1, -38 * P + 1]
    return [limbs(v) for v in vals] + [limbs(rand_val(rng, s)) for s in (1, 6, 38) for _ in range(n // 3)]


# ---------------------------------------------------------------- 32-bit-limb Montgomery fields (mont32.hpp)

def words32(v, n):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def mont_columns(a, b, p, n):
    """The product-scanning columns of fe_mul_body on integers: for every column k = 0 .. 2n - 2 the number of times the 64-bit
    accumulator wraps (what the carry word c2 must collect), and the digits m_k."""
    A, B, Pw = words32(a, n), words32(b, n), words32(p, n)
    inv = (-pow(p, -1, 1 << 32)) % (1 << 32)
    m, wraps, carry = [], [], 0
    for k in range(2 * n - 1):
        s = carry + sum(A[i] * B[k - i] for i in range(max(0, k - n + 1), min(k, n - 1) + 1))
        s += sum(m[i] * Pw[k - i] for i in range(max(0, k - n + 1), min(k, n)))
        if k < n:
            m.append((s * inv) & 0xffffffff)
            s += m[k] * Pw[0]
            assert s & 0xffffffff == 0
        wraps.append(s >> 64)           # the carry in is below 2^64: every wrap happens while the column's terms are added
        carry = s >> 32
    return wraps, m


def mont_operands(p, n, seed):
    """operand pairs below the modulus (the contract of fe_mul): edge values in every pair, limbs all 0xffffffff wherever the modulus
    allows, runs of zero limbs, single-limb spikes, pairs chosen by the carries of the 64-bit column accumulator, pairs whose Montgomery
    digits m_k are all 0 or all 0xffffffff, and random pairs.  Returns (singles, pairs, named) with named = {label: pair}."""
    rng = random.Random(seed)
    R = 1 << (32 * n)
    top = p >> (32 * (n - 1))
    ones_below = ((top - 1) << (32 * (n - 1))) | ((1 << (32 * (n - 1))) - 1)     # the largest value below p with all lower limbs 0xffffffff
    edge = [0, 1, 2, p - 1, p - 2, R % p, R * R % p, (p - 1) // 2, (p + 1) // 2, ones_below, (1 << (32 * (n - 1))) - 1]
    for run in range(1, n):                      # runs of zero limbs at the bottom, at the top and in the middle
        edge += [(ones_below >> (32 * run)) << (32 * run), ones_below & ((1 << (32 * run)) - 1)]
        edge.append(ones_below & ~(((1 << (32 * run)) - 1) << (32 * ((n - run) // 2))))
    for i in range(n):                           # single-limb spikes
        edge.append((0xffffffff if i < n - 1 else top - 1) << (32 * i))
        edge.append(1 << (32 * i))
    edge = [e for e in dict.fromkeys(edge) if 0 <= e < p]
    pairs = [(a, b) for a in edge for b in edge]
    named = {}
    # the 64-bit accumulator of column k wraps into c2 or not: in the first column, in the last column the contract allows, in none
    # (Fp: column 0 wraps on a_0 b_0 + m_0 p_0 alone; Fr has p_0 = 1, so a_0 b_0 + m_0 < 2^64 and its first such column is 1.  The
    # top limbs of operands below p are small: the last columns cannot wrap in either field.)
    cols = {(a, b): mont_columns(a, b, p, n)[0] for a in edge + [0xffffffff] for b in edge + [0xffffffff]}
    first_k = min(k for w in cols.values() for k, x in enumerate(w) if x)
    last_k = max(k for w in cols.values() for k, x in enumerate(w) if x)
    named["c2_first_column_%d" % first_k] = next(ab for ab, w in cols.items() if w[first_k])
    named["c2_last_column_%d" % last_k] = next(ab for ab, w in cols.items() if w[last_k])
    named["c2_most_columns"] = max(cols, key=lambda ab: sum(1 for x in cols[ab] if x))
    named["c2_no_column"] = next(ab for ab, w in cols.items() if min(ab) > 1 and not any(w))
    # Montgomery digits all 0 / all 0xffffffff / half and half: b = target / a mod 2^(32 n), kept when b < p
    for label, m in (("digits_zero", 0), ("digits_ones", R - 1), ("digits_low_ones", (1 << (16 * n)) - 1), ("digits_high_ones", R - (1 << (16 * n)))):
        target = -m * p % R
        for j in range(3):
            while True:
                a = rng.randrange(1, p) | 1
                b = target * pow(a, -1, R) % R
                if b < p:
                    break
            assert (-(a * b) * pow(p, -1, R)) % R == m
            named["%s_%d" % (label, j)] = (a, b)
    pairs += list(named.values())
    pairs += [(rng.randrange(p), rng.randrange(p)) for _ in range(3000)]
    singles = edge + [rng.randrange(p) for _ in range(1000)]
    return singles, pairs, named
