"""The two bodies of the 28-bit-limb Montgomery product (curdleproofs_amd/csrc/fp28.hpp): schoolbook and Karatsuba, compiled
for the host.  Both are checked against Python integers and against each other (they sum the same integer columns, so their
limbs must agree bit for bit), on random operands at 1, 12 and 38 p, on limbs driven to +-(2^28 - 1) with the top limb at its
largest lazy value, and on operands shaped like those that reach products in the point formulas of g1_28.hpp."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "host_emul", "emul.cpp")
BODIES = os.path.join(HERE, "host_emul", "f28_bodies.cpp")
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R392 = 1 << 392
MASK = (1 << 28) - 1
TOP38 = (38 * P) >> 364          # top limb of a value at the largest operand magnitude of the point formulas (38 p)


def _compile(src, out, defines=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread"] + ["-D" + d for d in defines] + ["-o", out, src])
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def bodies(tmp_path_factory):
    L = _compile(BODIES, str(tmp_path_factory.mktemp("f28b") / "f28_bodies.so"))
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    for f in (L.f28b_mul, L.f28b_mul_regs, L.f28b_mulsub):
        f.argtypes = [ctypes.c_int, vp, vp, sz]
        f.restype = None
    return L


@pytest.fixture(scope="module", params=[0, 1], ids=["school", "kara"])
def emul(request, tmp_path_factory):
    """tests/host_emul/emul.cpp with the given body as the default of every product (CPX_F28_KARATSUBA)."""
    L = _compile(EMUL, str(tmp_path_factory.mktemp("emul") / "emul.so"), ["CPX_F28_KARATSUBA=%d" % request.param])
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.emul_f28_mul.argtypes = [vp, vp, vp, sz]
    L.emul_f28_mulsub.argtypes = [vp, vp, vp, vp, vp, sz, ctypes.c_int]
    return L


def limbs(v):
    """normalised limbs of an integer: 0..12 in [0, 2^28), the top limb signed"""
    out = []
    for _ in range(13):
        out.append(v & MASK)
        v >>= 28
    return out + [v]


def value(ls):
    return sum(x << (28 * i) for i, x in enumerate(ls))


def _arr(rows):
    flat = [x for r in rows for ls in r for x in ls]
    return (ctypes.c_int32 * len(flat))(*flat)


def run(L, fn, kara, rows):
    n = len(rows)
    out = (ctypes.c_int32 * (14 * n))()
    getattr(L, fn)(kara, _arr(rows), out, n)
    return [list(out[14 * i:14 * i + 14]) for i in range(n)]


def check_montgomery(t, target):
    """t = (target + M p) / 2^392 for an integer M in [0, 2^392), with normalised limbs"""
    assert all(0 <= x <= MASK for x in t[:13])
    num = value(t) * R392 - target
    assert num % P == 0
    assert 0 <= num // P < R392


def check_both(L, rows):
    """schoolbook and Karatsuba bodies (and the out-of-line entry for products): exact Montgomery results, identical limbs"""
    if len(rows[0]) == 2:
        ref = run(L, "f28b_mul", 0, rows)
        for fn in ("f28b_mul", "f28b_mul_regs"):
            assert run(L, fn, 1, rows) == ref, fn
        assert run(L, "f28b_mul_regs", 0, rows) == ref
        for (a, b), t in zip(rows, ref):
            check_montgomery(t, value(a) * value(b))
    else:
        ref = run(L, "f28b_mulsub", 0, rows)
        assert run(L, "f28b_mulsub", 1, rows) == ref
        for (a, b, c, d), t in zip(rows, ref):
            check_montgomery(t, value(a) * value(b) - value(c) * value(d))


def rand_val(rng, scale):
    return rng.randrange(-scale * P, scale * P + 1)


def lazy_diff(x, y):
    """f28_sub_lazy: limb-wise difference of two normalised values, no carry pass"""
    return [p - q for p, q in zip(limbs(x), limbs(y))]


def test_random_operands_at_1_12_38_p(bodies):
    rng = random.Random(2028)
    for scale in (1, 12, 38):
        check_both(bodies, [[limbs(rand_val(rng, scale)), limbs(rand_val(rng, scale))] for _ in range(300)])
        check_both(bodies, [[limbs(rand_val(rng, scale)) for _ in range(4)] for _ in range(300)])


def test_extreme_limbs(bodies):
    """limbs at +-(2^28 - 1) (normalised maxima and the extremes of lazy differences / negations), top limb at its largest
    lazy value for 38 p, in every sign combination, and single-limb spikes on either half of the Karatsuba split"""
    pos = [MASK] * 13 + [TOP38]
    neg = [-MASK] * 13 + [-TOP38]
    alt = [MASK if i % 2 else -MASK for i in range(13)] + [TOP38]
    halves = [[MASK] * 7 + [-MASK] * 6 + [-TOP38], [-MASK] * 7 + [MASK] * 6 + [TOP38]]
    ops = [pos, neg, alt, [-x for x in alt]] + halves + [[0] * 14, limbs(P), limbs(P - 1)]
    spikes = []
    for i in range(14):
        s = [0] * 14
        s[i] = TOP38 if i == 13 else MASK
        spikes += [s, [-x for x in s]]
    ops += spikes
    check_both(bodies, [[a, b] for a in ops for b in ops])
    rng = random.Random(7)
    check_both(bodies, [[rng.choice(ops) for _ in range(4)] for _ in range(2000)])
    # the four operands of a difference all at the extreme of the same sign: the largest column sums of f28_mulsub_body
    check_both(bodies, [[pos, pos, neg, pos], [neg, neg, pos, neg], [pos, neg, neg, neg], [alt, alt, [-x for x in alt], alt]])


def test_operands_of_the_point_formulas(bodies):
    """operands shaped as in xyzz28_add_mixed_t, jac28_dbl and xyzz28_add (g1_28.hpp): products in (-0.81 p, 1.81 p),
    stored coordinates up to 15.4 p, lazy differences of a product and a coordinate, lazily negated y, shifted values"""
    rng = random.Random(381)
    prod = lambda: rng.randrange(-81 * P // 100, 181 * P // 100)
    coord = lambda m: rng.randrange(-int(m * P), int(m * P))
    cneg_lazy = lambda v: [-x for x in limbs(v)]
    rows2, rows4 = [], []
    for _ in range(300):
        # mixed addition: U2 = X2 ZZ1, S2 = (+-Y2) ZZZ1 (y lazily negated), P = U2 - X1, R = S2 - Y1 (lazy), PP = P^2, PPP = P PP,
        # Q = X1 PP, ZZZ3 = ZZZ1 PPP, Y3 = R (Q - X3) - Y1 PPP
        x2, y2, zz1, zzz1, x1, y1 = prod(), prod(), prod(), prod(), coord(6.3), coord(2.7)
        pp_, rr = lazy_diff(prod(), x1), lazy_diff(prod(), y1)
        pp2, ppp, qq, x3 = prod(), prod(), prod(), coord(6.3)
        rows2 += [[limbs(x2), limbs(zz1)], [cneg_lazy(y2), limbs(zzz1)], [limbs(zz1), limbs(pp2)], [pp_, limbs(pp2)],
                  [limbs(x1), limbs(pp2)], [limbs(zzz1), limbs(ppp)], [rr, rr], [pp_, pp_]]
        rows4 += [[rr, lazy_diff(qq, x3), limbs(y1), limbs(ppp)]]
        # Jacobian doubling: Y3 = E (D - X3) - (8 B) B with E = 3 A (A a square), D = 4 X B
        e, d, x3d, b = 3 * prod(), 4 * prod(), coord(15.4), prod()
        rows4 += [[limbs(e), lazy_diff(d, x3d), limbs(8 * b), limbs(b)]]
        # full XYZZ addition: R = S2 - S1 (lazy, both products), Y3 = R (Q - X3) - S1 PPP
        s1 = prod()
        rows4 += [[lazy_diff(prod(), s1), lazy_diff(prod(), coord(8.1)), limbs(s1), limbs(prod())]]
        rows2 += [[lazy_diff(prod(), s1), lazy_diff(prod(), prod())]]
    check_both(bodies, rows2)
    check_both(bodies, rows4)


def _to_mont(x):
    return (x * (1 << 384) % P).to_bytes(48, "little")


def _from_mont(b):
    return int.from_bytes(b, "little") * pow(1 << 384, -1, P) % P


def test_emul_products_against_integers(emul):
    """emul_f28_mul / emul_f28_mulsub of the emulation library built with each body as the default"""
    rng = random.Random(12)
    vals = [rng.randrange(P) for _ in range(150)] + [0, 1, P - 1, P - 2, 1 << 380, (P - 1) // 2]
    rot = lambda k: vals[k:] + vals[:k]
    enc = lambda vs: b"".join(_to_mont(v) for v in vs)
    buf = lambda b: (ctypes.c_uint8 * len(b)).from_buffer_copy(b)
    o = (ctypes.c_uint8 * (48 * len(vals)))()
    emul.emul_f28_mul(buf(enc(vals)), buf(enc(rot(3))), o, len(vals))
    assert [_from_mont(bytes(o)[48 * i:48 * i + 48]) for i in range(len(vals))] == [x * y % P for x, y in zip(vals, rot(3))]
    a, b, c, d = vals, rot(1), rot(7), rot(13)
    for scale in (1, 12, 38):
        emul.emul_f28_mulsub(buf(enc(a)), buf(enc(b)), buf(enc(c)), buf(enc(d)), o, len(vals), scale)
        got = [_from_mont(bytes(o)[48 * i:48 * i + 48]) for i in range(len(vals))]
        assert got == [(scale * scale * (w * x - y * z)) % P for w, x, y, z in zip(a, b, c, d)], scale
