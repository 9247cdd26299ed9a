"""CPU checks of the request lists that take the prover's R and S from the per-proof tables (curdleproofs_amd/csrc/prove_reqs.hpp:
prove_rs_tables, prove_rs_sums; option rs_from_tables): which rows, how many entries, which scalars, which slots — written from the
protocol, not read back from the header — and, with the oracle's group arithmetic, the identity the lists rest on:
msm(vec_T, a_sigma) = k msm(vec_R, a) and msm(vec_U, a_sigma) = k msm(vec_S, a) for a witness with T = k sigma(R), U = k sigma(S).
The lists are compiled with the host compiler by tests/host_emul/rs_tables_emul.cpp."""
import ctypes
from collections import namedtuple

import pytest

from tests.check_harness import build_emul
from tests.oracle_lib import AFF, FR

NAMES = ("SL_R SL_S SL_CMT2 SL_CMU2 CMA2 CMB2 TMP0 NSLOTS D T U NROW V_APERM V_COUNT SEG_NONE SEG_PTAB GA_NONE SCAL_NONE SCAL_VEC "
         "SC_K_INV SC_RK_K_INV SC_XFIN SC_COUNT RK SLOT_RK SLOT_SK N_BLINDERS").split()
RS_TABLES, RS_SUMS, P1T, P1 = range(4)
SHAPES = [(8, 3), (32, 5), (256, 8)]   # ell = 4, 28 (the oracle tests' smallest shape), 252 (the benchmark's)

Seg = namedtuple("Seg", "kind gather off n arg")
Req = namedtuple("Req", "seg0 seg1 scal_kind scal_at keep out add")


@pytest.fixture(scope="module")
def lib():
    return ctypes.CDLL(build_emul("rs_tables_emul.cpp", ["prove_reqs.hpp", "layout.hpp", "protocol.h", "mont32.hpp"], shared=True))


class Shape:
    def __init__(self, lib, n, L):
        self.lib, self.n, self.L = lib, n, L
        buf = (ctypes.c_int32 * 64)()
        cnt = lib.rs_consts(n, L, buf)
        assert cnt == len(NAMES)
        self.__dict__.update(zip(NAMES, buf[:cnt]))

    def reqs(self, which):
        buf = (ctypes.c_int32 * (17 * 16))()
        cnt = self.lib.rs_list(which, self.n, self.L, buf)
        out = []
        for i in range(cnt):
            v = list(buf[17 * i:17 * i + 17])
            out.append(Req(Seg(*v[0:5]), Seg(*v[5:10]), v[10], v[11], v[12], v[13], tuple(a for a in v[14:17] if a >= 0)))
        return out


@pytest.fixture(scope="module", params=SHAPES, ids=["ell4", "ell28", "ell252"])
def sh(lib, request):
    return Shape(lib, *request.param)


def test_the_two_msm_requests(sh):
    ell = sh.n - 4
    assert sh.N_BLINDERS == 4
    rs = sh.reqs(RS_TABLES)
    assert len(rs) == 2
    for r, row_at, keep in zip(rs, (sh.T, sh.U), (sh.SLOT_RK, sh.SLOT_SK)):
        # the proof's table row from T() / U() on, in the given order (no gather list), the first ell entries: not the four blinder slots
        assert r.seg0 == Seg(sh.SEG_PTAB, sh.GA_NONE, row_at, ell, 0)
        assert r.seg1.kind == sh.SEG_NONE and r.seg1.n == 0
        # the scalars: a_sigma (V_APERM), whose first ell entries are the permuted vec_a
        assert (r.scal_kind, r.scal_at) == (sh.SCAL_VEC, sh.V_APERM) and 0 <= sh.V_APERM < sh.V_COUNT
        assert r.keep == keep and r.out == -1 and r.add == ()
    # both rows lie inside a proof's row of the table: T occupies [T, T + n), U [U, U + n)
    assert sh.U == sh.T + sh.n and sh.U + sh.n == sh.NROW
    # phase 1t reads the same rows with all n entries: the new requests stop four short of it
    p1t = sh.reqs(P1T)
    assert [(r.seg0.off, r.seg0.n) for r in p1t] == [(sh.T, sh.n), (sh.U, sh.n)]


def test_the_kept_points_have_slots_of_their_own(sh):
    tmp = [sh.TMP0 + i for i in range(8)]
    assert sh.SLOT_RK != sh.SLOT_SK and {sh.SLOT_RK, sh.SLOT_SK} <= set(tmp) and tmp[-1] == sh.NSLOTS - 1
    # TMP(0..3) keep r * H of phase 1 (read by the side stream at the same time); TMP(5) and TMP(7) are the write-only slots of the plans
    p1_kept = {r.keep for r in sh.reqs(P1) if r.keep >= 0}
    assert not {sh.SLOT_RK, sh.SLOT_SK} & (p1_kept | {tmp[5], tmp[7]})
    assert {tmp[q] for q in range(4)} <= p1_kept
    # no proof point lives there
    assert min(sh.SLOT_RK, sh.SLOT_SK) > sh.D
    # the side stream's scalars k^-1 and r_k k^-1 have entries of their own among the small scalars
    assert sh.SC_XFIN < sh.SC_K_INV < sh.SC_RK_K_INV < sh.SC_COUNT


def test_the_two_sums(sh):
    sums = sh.reqs(RS_SUMS)
    assert len(sums) == 2
    # cm_T.T_2 = k R + r_t H = Rk + TMP(0), cm_U.T_2 = k S + r_u H = Sk + TMP(1): no bases, no scalars, two addends with coefficient 1
    for r, kept, rh, out in zip(sums, (sh.SLOT_RK, sh.SLOT_SK), (sh.TMP0, sh.TMP0 + 1), (sh.SL_CMT2, sh.SL_CMU2)):
        assert r.seg0.kind == r.seg1.kind == sh.SEG_NONE and r.seg0.n == r.seg1.n == 0 and r.scal_kind == sh.SCAL_NONE
        assert r.add == (kept, rh) and r.out == out and r.keep == out
    # together with the four scalar multiplications the six points of the side stream are covered, each once
    side = (ctypes.c_int32 * 6)()
    sh.lib.rs_side_slots(sh.L, side)
    assert sorted(side) == sorted([sh.SL_R, sh.SL_S, sh.CMA2, sh.CMB2] + [r.out for r in sums])


@pytest.mark.parametrize("seed", [0, 5])
def test_the_sums_over_the_tables_are_k_times_r_and_s(orc, seed):
    """A small oracle instance (ell = 28): with a_sigma(j) = a[permutation[j]], as k_ps_aperm fills V_APERM, msm(vec_T, a_sigma) is
    k msm(vec_R, a) and msm(vec_U, a_sigma) is k msm(vec_S, a) — for ANY vec_a, so a fixed one serves.  With the scalars left
    unpermuted (vec_a itself) the sums differ: the permutation belongs to the scalars."""
    ell = 28
    crs = orc.generate_crs_points(ell)
    inst = orc.make_instance(ell, seed, crs)
    perm = inst["permutation"]
    assert sorted(perm) == list(range(ell)) and perm != list(range(ell))
    a = [orc.fr_from_u64(1000003 * i + 17) for i in range(ell)]
    a_sigma = b"".join(a[perm[j]] for j in range(ell))
    vec_a = b"".join(a)
    assert len(vec_a) == ell * FR and len(inst["vec_T"]) == ell * AFF
    for base, image in (("vec_R", "vec_T"), ("vec_S", "vec_U")):
        plain = orc.g1_to_affine(orc.g1_msm(inst[base], vec_a))            # R = msm(vec_R, a) (curdleproofs.rs:112-113)
        want = orc.g1_compress(orc.g1_scale(plain, inst["k"]))             # k R
        got = orc.g1_compress_jac(orc.g1_msm(inst[image], a_sigma))
        assert got == want
        assert orc.g1_compress_jac(orc.g1_msm(inst[image], vec_a)) != want
        # ... and back: R = k^-1 (k R)
        back = orc.g1_scale(orc.g1_decompress(got), orc.fr_inv(inst["k"]))
        assert orc.g1_compress(back) == orc.g1_compress(plain)
