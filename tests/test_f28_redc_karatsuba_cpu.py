"""The Karatsuba Montgomery half and the Karatsuba square of the 28-bit-limb field (curdleproofs_amd/csrc/fp28.hpp), compiled for
the host.  Every body (schoolbook; Karatsuba a b with the schoolbook reduction; Karatsuba a b with the Karatsuba reduction) and
both squares are checked against Python integers and against each other: they sum the same integer columns, so their limbs must
agree bit for bit.  Operands: random values at 1, 12 and 38 p, limbs driven to +-(2^28 - 1) with the top limb at its largest
lazy value, f28_sub_lazy / f28_cneg_lazy shapes and the operand shapes of the point formulas of g1_28.hpp.  The emulation
library (tests/host_emul/emul.cpp) built with each reduction as the default runs the point-level checks."""
import ctypes
import os
import random
import subprocess

import pytest

from tests.f28_vectors import P, RMOD, check_montgomery, extreme_sets, lazy_shape_sets, point_formula_sets, random_sets, value

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "host_emul", "emul.cpp")
BODIES = os.path.join(HERE, "host_emul", "f28_redc_bodies.cpp")
SCHOOL, KARA_AB, KARA_REDC, DEFAULT = 0, 1, 2, -1
AFF, FR = 96, 32


def _compile(src, out, defines=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread"] + ["-D" + d for d in defines] + ["-o", out, src])
    return ctypes.CDLL(out)


def _bind(L):
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    for f in (L.f28r_mul, L.f28r_sqr):
        f.argtypes = [ci, ci, vp, vp, sz]
        f.restype = None
    L.f28r_mulsub.argtypes = [ci, vp, vp, sz]
    L.f28r_mulsub.restype = None
    L.f28r_defaults.restype = ci
    return L


@pytest.fixture(scope="module")
def bodies(tmp_path_factory):
    return _bind(_compile(BODIES, str(tmp_path_factory.mktemp("f28r") / "f28_redc_bodies.so")))


def _arr(flat):
    return (ctypes.c_int32 * len(flat))(*flat)


def run_mul(L, body, regs, rows):
    n = len(rows)
    out = (ctypes.c_int32 * (14 * n))()
    L.f28r_mul(body, regs, _arr([x for r in rows for ls in r for x in ls]), out, n)
    return [list(out[14 * i:14 * i + 14]) for i in range(n)]


def run_mulsub(L, body, rows):
    n = len(rows)
    out = (ctypes.c_int32 * (14 * n))()
    L.f28r_mulsub(body, _arr([x for r in rows for ls in r for x in ls]), out, n)
    return [list(out[14 * i:14 * i + 14]) for i in range(n)]


def run_sqr(L, body, regs, ops):
    n = len(ops)
    out = (ctypes.c_int32 * (14 * n))()
    L.f28r_sqr(body, regs, _arr([x for ls in ops for x in ls]), out, n)
    return [list(out[14 * i:14 * i + 14]) for i in range(n)]


def check_products(L, rows):
    ref = run_mul(L, SCHOOL, 0, rows)
    for body in (KARA_AB, KARA_REDC, DEFAULT):
        for regs in (0, 1):
            assert run_mul(L, body, regs, rows) == ref, (body, regs)
    for (a, b), t in zip(rows, ref):
        check_montgomery(t, value(a) * value(b))


def check_differences(L, rows):
    ref = run_mulsub(L, SCHOOL, rows)
    for body in (KARA_AB, KARA_REDC, DEFAULT):
        assert run_mulsub(L, body, rows) == ref, body
    for (a, b, c, d), t in zip(rows, ref):
        check_montgomery(t, value(a) * value(b) - value(c) * value(d))


def check_squares(L, ops):
    ref = run_sqr(L, SCHOOL, 0, ops)
    assert run_mul(L, SCHOOL, 0, [[a, a] for a in ops]) == ref   # a square sums the columns of a a
    for body in (KARA_REDC, DEFAULT):
        for regs in (0, 1):
            assert run_sqr(L, body, regs, ops) == ref, (body, regs)
    for a, t in zip(ops, ref):
        check_montgomery(t, value(a) ** 2)


def test_defaults_select_the_karatsuba_reduction(bodies):
    assert bodies.f28r_defaults() == 7


def test_random_operands_at_1_12_38_p(bodies):
    for _, ops, rows2, rows4 in random_sets():
        check_squares(bodies, ops)
        check_products(bodies, rows2)
        check_differences(bodies, rows4)


def test_extreme_limbs(bodies):
    """limbs at +-(2^28 - 1), top limb at its largest lazy value for 38 p, in every sign combination, single-limb spikes on
    either half of the split, and values whose Montgomery digits come out at 0 or 2^28 - 1 (the extremes of dm_i)"""
    e = extreme_sets()
    check_squares(bodies, e["squares"])
    check_products(bodies, e["pairs"])
    check_differences(bodies, e["fours"])
    # the largest column sums of f28_mulsub_body: all four operands at the extreme of the same sign
    check_differences(bodies, e["same_sign"])
    # products whose Montgomery digits (m = -a b p^-1 mod 2^392) are 0, all 2^28 - 1, or one half all 2^28 - 1 and the other 0:
    # dm_i = m_i - m_(7+i) and the substituted m_(k-7) dP_0 of the Karatsuba reduction at both ends of their range
    check_products(bodies, e["digit_rows"])
    check_differences(bodies, e["digit_fours"])


def test_lazy_difference_and_negation_shapes(bodies):
    """f28_sub_lazy / f28_cneg_lazy results as operands: limbs in (-2^28, 2^28) of either sign, top limb signed"""
    ops, rows2, rows4 = lazy_shape_sets()
    check_squares(bodies, ops)
    check_products(bodies, rows2)
    check_differences(bodies, rows4)


def test_operands_of_the_point_formulas(bodies):
    """operands shaped as in xyzz28_add_mixed_t, jac28_dbl, xyzz28_dbl and xyzz28_add (g1_28.hpp): products in (-0.81 p, 1.81 p),
    stored coordinates up to 15.4 p, lazy differences of a product and a coordinate, lazily negated y, shifted values"""
    sq, rows2, rows4 = point_formula_sets()
    check_products(bodies, rows2)
    check_differences(bodies, rows4)
    check_squares(bodies, sq)


@pytest.fixture(scope="module", params=[0, 1], ids=["redc_school", "redc_kara"])
def emul(request, tmp_path_factory):
    """tests/host_emul/emul.cpp with the given reduction as the default of every product and square (CPX_F28_REDC_KARATSUBA)"""
    L = _compile(EMUL, str(tmp_path_factory.mktemp("emulr") / "emul.so"), ["CPX_F28_REDC_KARATSUBA=%d" % request.param])
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.emul_f28_mul.argtypes = [vp, vp, vp, sz]
    L.emul_f28_mulsub.argtypes = [vp, vp, vp, vp, vp, sz, ctypes.c_int]
    L.emul_f28_msm.argtypes = [vp, vp, sz, vp, vp]
    L.emul_f28_xyzz_sum.argtypes = [vp, sz, vp, vp, vp]
    L.emul_f28_xyzz_full.argtypes = [vp, sz, vp, vp, vp]
    L.emul_msm_endo.argtypes = [vp, vp, sz, ctypes.c_int, vp]
    L.emul_msm_endo.restype = None
    return L


def _b(x):
    return (ctypes.c_uint8 * len(x)).from_buffer_copy(x)


def _to_mont(x):
    return (x * (1 << 384) % P).to_bytes(48, "little")


def _from_mont(b):
    return int.from_bytes(b, "little") * pow(1 << 384, -1, P) % P


def test_emul_field_against_integers(emul):
    rng = random.Random(21)
    vals = [rng.randrange(P) for _ in range(150)] + [0, 1, P - 1, P - 2, 1 << 380, (P - 1) // 2]
    rot = lambda k: vals[k:] + vals[:k]
    enc = lambda vs: _b(b"".join(_to_mont(v) for v in vs))
    o = (ctypes.c_uint8 * (48 * len(vals)))()
    emul.emul_f28_mul(enc(vals), enc(rot(5)), o, len(vals))
    assert [_from_mont(bytes(o)[48 * i:48 * i + 48]) for i in range(len(vals))] == [x * y % P for x, y in zip(vals, rot(5))]
    a, b, c, d = vals, rot(2), rot(9), rot(17)
    for scale in (1, 12, 38):
        emul.emul_f28_mulsub(enc(a), enc(b), enc(c), enc(d), o, len(vals), scale)
        got = [_from_mont(bytes(o)[48 * i:48 * i + 48]) for i in range(len(vals))]
        assert got == [(scale * scale * (w * x - y * z)) % P for w, x, y, z in zip(a, b, c, d)], scale


def test_emul_point_formulas(emul, orc):
    """Jacobian double-and-add, XYZZ bucket accumulation (the inlined mixed addition of the bucket loops), the full XYZZ addition
    and the table MSM of the prover, in the kernels' arithmetic with the selected default, against the oracle"""
    rng = orc.rng(4242)
    n = 6
    bases, scalars = rng.g1_affine(n), rng.fr(n)
    o = (ctypes.c_uint8 * AFF)()
    mags = (ctypes.c_double * 3)()
    emul.emul_f28_msm(_b(bases), _b(scalars), n, o, mags)
    assert bytes(o) == orc.g1_to_affine(orc.g1_msm(bases, scalars, naive=True))
    assert mags[0] <= 15.4 and mags[1] <= 15.4 and mags[2] <= 3.6, list(mags)
    # bucket accumulation with repeated and opposite points
    pts = [rng.g1_affine(1) for _ in range(40)]
    seq = pts + [pts[3], pts[3], pts[7]]
    signs = bytes([(i * 3 + i // 5) & 1 for i in range(40)] + [0, 1, 1 - ((7 * 3 + 1) & 1)])
    emul.emul_f28_xyzz_sum(_b(b"".join(seq)), len(seq), _b(signs), o, mags)
    rm1 = orc.fr_from_canonical_bytes((RMOD - 1).to_bytes(32, "little"))
    scal = b"".join(rm1 if s else orc.fr_from_u64(1) for s in signs)
    assert bytes(o) == orc.g1_to_affine(orc.g1_msm(b"".join(seq), scal, naive=True))
    assert mags[0] <= 6.3 and mags[1] <= 2.7, list(mags)
    # full XYZZ addition, chain and tree, and its exceptional cases
    m = 16
    fb = b"".join(pts[:m])
    fs = bytes([i % 3 == 0 for i in range(m)])
    out = (ctypes.c_uint8 * (8 * AFF))()
    emul.emul_f28_xyzz_full(_b(fb), m, _b(fs), out, mags)
    got = [bytes(out)[i * AFF:(i + 1) * AFF] for i in range(8)]
    total = orc.g1_to_affine(orc.g1_msm(fb, b"".join(rm1 if s else orc.fr_from_u64(1) for s in fs), naive=True))
    k0 = (RMOD - 1) if fs[0] else 1
    mult = lambda k: orc.g1_to_affine(orc.g1_msm(pts[0], orc.fr_from_canonical_bytes((k * k0 % RMOD).to_bytes(32, "little")), naive=True))
    assert got[0] == total and got[1] == total
    assert got[2:] == [mult(2), bytes(AFF), mult(1), mult(1), mult(2), mult(3)]
    # the table MSM of the prover (k_table_build + k_msm_tblw + the weighted reductions)
    n = 12
    bases, scalars = rng.g1_affine(n), rng.fr(n)
    j = (ctypes.c_uint8 * 144)()
    emul.emul_msm_endo(_b(bases), _b(scalars), n, 0, j)
    assert orc.g1_compress_jac(bytes(j)) == orc.g1_compress_jac(orc.g1_msm(bases, scalars, naive=True))
