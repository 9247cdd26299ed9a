"""CPU checks of the protocol's table-backed MSM requests (curdleproofs_amd/csrc/prove_reqs.hpp): the ONE list that the host-driven
prover / verifier and the device-resident plans materialise.  Compiled with the host compiler by tests/host_emul/prove_reqs_emul.cpp,
which flattens the descriptors into integers; everything asserted here is written from the protocol's tables of requests — which
bases, which scalars, which kept point, which output slot, which addends — not read back from the header."""
import ctypes
from collections import Counter, namedtuple

import pytest

from tests.check_harness import build_emul

NAMES = ("SL_A SL_CMT1 SL_CMT2 SL_CMU1 SL_CMU2 SL_R SL_S SL_B SL_C SL_BC SL_BD CMA1 CMA2 CMB1 CMB2 BA BT BU D APRIME TMP0 NSLOTS NPOINTS "
         "VR IR RT RU RA RB NRAND M T U H G_t G_u G_sum H_sum V_APERM V_FACT V_C V_ZZU V_COUNT SC_BETA_SP SC_ALPHA_SP SC_NEG_BETA_G_INV SC_ALPHA_G "
         "SC_COUNT VSC_NEG_BETA_G_INV VSC_ALPHA_G VSC_COUNT SEG_NONE SEG_CRS SEG_PTAB GA_NONE GA_BASIS GA_HI GA_LO GA_BASIS_HI GA_BASIS_LO GA_COL "
         "GA_HI_H GA_LO_H SCAL_NONE SCAL_RAND SCAL_VEC SCAL_SC SCAL_ROUND").split()
P1B, P1, P1T, P2, P2_COMMIT, P3, IPA, IPA_FUSED, SMSM, VERIFY = range(10)
# ell = 4: the smallest shape with more than one round, and a `half` of 1; ell = 28: the README example
SHAPES = [(8, 3), (32, 5)]

Seg = namedtuple("Seg", "kind gather off n arg")
Req = namedtuple("Req", "seg0 seg1 scal_kind scal_at keep out add")


@pytest.fixture(scope="module")
def lib():
    return ctypes.CDLL(build_emul("prove_reqs_emul.cpp", ["prove_reqs.hpp", "layout.hpp", "protocol.h", "mont32.hpp"], shared=True))


class Shape:
    """One (n, L): the layout's names and the request lists, as plain Python values."""

    def __init__(self, lib, n, L):
        self.lib, self.n, self.L, self.hn = lib, n, L, n // 2
        buf = (ctypes.c_int32 * 128)()
        cnt = lib.pr_consts(n, L, buf)
        assert cnt == len(NAMES)
        self.__dict__.update(zip(NAMES, buf[:cnt]))
        basis = (ctypes.c_uint32 * n)()
        lib.pr_basis(n, basis)
        self.basis = list(basis)

    def TMP(self, i):
        return self.TMP0 + i

    def slot(self, which, j):
        return self.lib.pr_slot_round(self.L, "LC RC LD RD LA LT LU RA RT RU".split().index(which), j)

    def half(self, j):
        return self.n >> (j + 1)

    def reqs(self, phase, j=0):
        buf, stride = (ctypes.c_int32 * (17 * 16))(), ctypes.c_int32()
        cnt = self.lib.pr_list(phase, self.n, self.L, j, buf, ctypes.byref(stride))
        assert 0 <= cnt <= 12
        out = []
        for i in range(cnt):
            v = list(buf[17 * i:17 * i + 17])
            out.append(Req(Seg(*v[0:5]), Seg(*v[5:10]), v[10], v[11], v[12], v[13], tuple(a for a in v[14:17] if a >= 0)))
            assert all(a == -1 for a in v[14 + len(out[-1].add):17]), "addends are packed to the front"
        return out, stride.value

    def gather(self, gather, arg):
        buf = (ctypes.c_uint32 * (self.n + 2))()
        return list(buf[:self.lib.pr_gather(self.n, gather, arg, buf)])

    def cols(self, seg):
        """The columns / row entries a segment reads, in order."""
        if seg.kind == self.SEG_NONE:
            assert seg.n == 0
            return []
        if seg.gather == self.GA_NONE:
            return list(range(seg.off, seg.off + seg.n))
        assert seg.off == 0 or seg.kind == self.SEG_PTAB   # (a table segment's gather list is relative to its row entry `off`)
        g = self.gather(seg.gather, seg.arg)
        assert len(g) == seg.n
        return g

    def hi(self, j):
        return [k for k in range(self.n) if k & self.half(j)]

    def lo(self, j):
        return [k for k in range(self.n) if not k & self.half(j)]


@pytest.fixture(scope="module", params=SHAPES, ids=["ell4", "ell28"])
def sh(lib, request):
    return Shape(lib, *request.param)


def _row(sh, r, kind0, cols0, kind1, cols1, scal_kind, scal_at, keep, out, add=()):
    assert (r.seg0.kind, sh.cols(r.seg0)) == (kind0, cols0)
    assert (r.seg1.kind, sh.cols(r.seg1)) == (kind1, cols1)
    assert (r.scal_kind, r.scal_at, r.keep, r.out, r.add) == (scal_kind, scal_at, keep, out, tuple(add))


def test_rows_of_the_commitment_phases(sh):
    n, crs, tab, none = sh.n, sh.SEG_CRS, sh.SEG_PTAB, sh.SEG_NONE
    G = list(range(n))
    (a,), _ = sh.reqs(P1B)
    _row(sh, a, crs, G, none, [], sh.SCAL_VEC, sh.V_APERM, sh.SL_A, sh.SL_A)
    assert a.seg0.gather == sh.GA_NONE
    p1, _ = sh.reqs(P1)
    assert len(p1) == 10
    _row(sh, p1[0], crs, G[:n - 2] + [sh.G_t, sh.G_u], none, [], sh.SCAL_RAND, sh.VR, -1, sh.BA)          # B_a over the SameMSM basis
    assert p1[0].seg0.gather == sh.GA_BASIS
    _row(sh, p1[1], crs, G, none, [], sh.SCAL_RAND, sh.IR, -1, sh.SL_BC)                                  # B_c
    assert p1[1].seg0.gather == sh.GA_NONE
    _row(sh, p1[2], crs, [sh.G_t], none, [], sh.SCAL_RAND, sh.RT, sh.SL_CMT1, sh.SL_CMT1)                 # cm_T.T_1
    _row(sh, p1[3], crs, [sh.G_u], none, [], sh.SCAL_RAND, sh.RU, sh.SL_CMU1, sh.SL_CMU1)                 # cm_U.T_1
    _row(sh, p1[4], crs, [sh.G_t], none, [], sh.SCAL_RAND, sh.RA, -1, sh.CMA1)                            # cm_A.T_1
    _row(sh, p1[5], crs, [sh.G_u], none, [], sh.SCAL_RAND, sh.RB, -1, sh.CMB1)                            # cm_B.T_1
    for q, draw in enumerate((sh.RT, sh.RU, sh.RA, sh.RB)):                                               # r * H: kept, never an output
        _row(sh, p1[6 + q], crs, [sh.H], none, [], sh.SCAL_RAND, draw, sh.TMP(q), -1)
    for r in p1[2:]:
        assert r.seg0.gather == sh.GA_COL, "the single CRS points are one-column gather lists"
    p1t, _ = sh.reqs(P1T)
    assert len(p1t) == 2
    _row(sh, p1t[0], tab, list(range(sh.T, sh.T + n)), none, [], sh.SCAL_RAND, sh.VR, -1, sh.BT)
    _row(sh, p1t[1], tab, list(range(sh.U, sh.U + n)), none, [], sh.SCAL_RAND, sh.VR, -1, sh.BU)
    p2, _ = sh.reqs(P2)
    assert len(p2) == 3
    _row(sh, p2[0], crs, [sh.G_sum], tab, [sh.M], sh.SCAL_SC, sh.SC_BETA_SP, sh.SL_B, sh.SL_B, (sh.SL_A,))   # B: beta on G_sum, alpha on M
    assert sh.SC_ALPHA_SP == sh.SC_BETA_SP + 1
    _row(sh, p2[1], none, [], none, [], sh.SCAL_NONE, 0, -1, sh.APRIME, (sh.SL_A, sh.SL_CMT1, sh.SL_CMU1))   # A'
    _row(sh, p2[2], crs, G, none, [], sh.SCAL_VEC, sh.V_C, -1, sh.SL_C)
    p2c, _ = sh.reqs(P2_COMMIT)
    _row(sh, p2c[0], crs, G, none, [], sh.SCAL_VEC, sh.V_FACT, sh.SL_B, sh.SL_B)                             # B in commitment form
    assert p2c[1:] == p2[1:]
    p3, _ = sh.reqs(P3)
    assert len(p3) == 2
    _row(sh, p3[0], crs, [sh.G_sum, sh.H_sum], none, [], sh.SCAL_SC, sh.SC_NEG_BETA_G_INV, -1, sh.D, (sh.SL_B,))
    assert sh.SC_ALPHA_G == sh.SC_NEG_BETA_G_INV + 1 and sh.H_sum == sh.G_sum + 1
    _row(sh, p3[1], crs, G, none, [], sh.SCAL_VEC, sh.V_ZZU, -1, sh.SL_BD)
    for r in (p2[0], p2[2], p2c[0], p3[0], p3[1]):
        assert r.seg0.gather == r.seg1.gather == sh.GA_NONE


def test_rows_of_the_rounds(sh):
    crs, tab, none, hn = sh.SEG_CRS, sh.SEG_PTAB, sh.SEG_NONE, sh.hn
    for j in range(sh.L):
        hi, lo = sh.hi(j), sh.lo(j)
        ipa, stride = sh.reqs(IPA, j)
        assert stride == 4 * hn + 2 and len(ipa) == 4
        _row(sh, ipa[0], crs, hi, crs, [sh.H], sh.SCAL_ROUND, 0, -1, sh.slot("LC", j))
        _row(sh, ipa[1], crs, lo, none, [], sh.SCAL_ROUND, hn + 1, -1, sh.slot("LD", j))
        _row(sh, ipa[2], crs, lo, crs, [sh.H], sh.SCAL_ROUND, 2 * hn + 1, -1, sh.slot("RC", j))
        _row(sh, ipa[3], crs, hi, none, [], sh.SCAL_ROUND, 3 * hn + 2, -1, sh.slot("RD", j))
        assert [r.seg0.gather for r in ipa] == [sh.GA_HI, sh.GA_LO, sh.GA_LO, sh.GA_HI]
        fused, stride = sh.reqs(IPA_FUSED, j)
        assert stride == 4 * hn + 2 and len(fused) == 4
        _row(sh, fused[0], crs, hi + [sh.H], none, [], sh.SCAL_ROUND, 0, -1, sh.slot("LC", j))
        _row(sh, fused[2], crs, lo + [sh.H], none, [], sh.SCAL_ROUND, 2 * hn + 1, -1, sh.slot("RC", j))
        assert (fused[1], fused[3]) == (ipa[1], ipa[3])
        smsm, stride = sh.reqs(SMSM, j)
        assert stride == 2 * hn and len(smsm) == 6
        for q, (name, left) in enumerate((("LA", True), ("LT", True), ("LU", True), ("RA", False), ("RT", False), ("RU", False))):
            half_list = hi if left else lo
            r = smsm[q]
            if q % 3 == 0:   # the A family: the SameMSM basis, composed with hi / lo
                _row(sh, r, crs, [sh.basis[k] for k in half_list], none, [], sh.SCAL_ROUND, 0 if left else hn, -1, sh.slot(name, j))
            else:            # T_b / U_b: the proof's table row from T() / U() on, through hi / lo
                _row(sh, r, tab, half_list, none, [], sh.SCAL_ROUND, 0 if left else hn, -1, sh.slot(name, j))
                assert (r.seg0.off, r.seg0.gather) == (sh.T if q % 3 == 1 else sh.U, sh.GA_HI if left else sh.GA_LO)


def test_rows_of_the_verifier(sh):
    v, _ = sh.reqs(VERIFY)
    assert len(v) == 2
    _row(sh, v[0], sh.SEG_CRS, [sh.G_sum, sh.H_sum], sh.SEG_NONE, [], sh.SCAL_SC, sh.VSC_NEG_BETA_G_INV, sh.D, sh.D, (sh.SL_B,))
    assert sh.VSC_ALPHA_G == sh.VSC_NEG_BETA_G_INV + 1
    _row(sh, v[1], sh.SEG_NONE, [], sh.SEG_NONE, [], sh.SCAL_NONE, 0, sh.APRIME, sh.APRIME, (sh.SL_A, sh.SL_CMT1, sh.SL_CMU1))
    assert v[0].scal_at + v[0].seg0.n + v[0].seg1.n <= sh.VSC_COUNT


def _all_phases(sh, commit, fused):
    """(phase name, requests, row stride) of one prove, in execution order: 1, 1b, 1t, 2, 3, the rounds."""
    out = [("1", *sh.reqs(P1)), ("1b", *sh.reqs(P1B)), ("1t", *sh.reqs(P1T)), ("2", *sh.reqs(P2_COMMIT if commit else P2)), ("3", *sh.reqs(P3))]
    out += [("ipa%d" % j, *sh.reqs(IPA_FUSED if fused else IPA, j)) for j in range(sh.L)]
    out += [("smsm%d" % j, *sh.reqs(SMSM, j)) for j in range(sh.L)]
    return out


@pytest.mark.parametrize("commit,fused", [(False, False), (True, False), (False, True), (True, True)])
def test_every_proof_point_is_an_output_exactly_once(sh, commit, fused):
    side = (ctypes.c_int32 * 6)()
    sh.lib.pr_side_slots(sh.L, side)
    assert list(side) == [sh.SL_R, sh.SL_S, sh.SL_CMT2, sh.SL_CMU2, sh.CMA2, sh.CMB2]
    outs = Counter(side)
    for _, reqs, _ in _all_phases(sh, commit, fused):
        outs.update(r.out for r in reqs if r.out >= 0)
    assert sh.D - sh.SL_A == sh.NPOINTS
    assert outs == Counter(list(range(sh.SL_A, sh.D)) + [sh.D, sh.APRIME]), "the proof points, D and A': each once, nothing else"
    assert not any(s >= sh.TMP0 for s in outs) and sh.TMP0 > sh.APRIME


def test_phase_1_with_a_leading(sh):
    outs = (ctypes.c_int32 * 16)()
    cnt = sh.lib.pr_then(sh.n, sh.L, outs)
    assert list(outs[:cnt]) == [sh.SL_A, sh.BA, sh.SL_BC, sh.SL_CMT1, sh.SL_CMU1, sh.CMA1, sh.CMB1, -1, -1, -1, -1]


@pytest.mark.parametrize("commit,fused", [(False, False), (True, True)])
def test_scalars_stay_inside_their_source(sh, commit, fused):
    for name, reqs, stride in _all_phases(sh, commit, fused):
        for r in reqs:
            cnt = r.seg0.n + r.seg1.n
            if r.scal_kind == sh.SCAL_NONE:
                assert cnt == 0
            elif r.scal_kind == sh.SCAL_RAND:
                assert 0 <= r.scal_at and r.scal_at + cnt <= sh.NRAND == 3 * sh.n + 9
            elif r.scal_kind == sh.SCAL_VEC:
                assert 0 <= r.scal_at < sh.V_COUNT and cnt <= sh.n
            elif r.scal_kind == sh.SCAL_SC:
                assert 0 <= r.scal_at and r.scal_at + cnt <= sh.SC_COUNT
            else:
                assert r.scal_kind == sh.SCAL_ROUND and name.startswith(("ipa", "smsm"))
                assert stride == (4 * sh.hn + 2 if name.startswith("ipa") else 2 * sh.hn)
                assert 0 <= r.scal_at and r.scal_at + cnt <= stride


@pytest.mark.parametrize("commit", [False, True])
def test_addends_name_kept_points_of_earlier_phases(sh, commit):
    kept, adds = set(), {}
    for name, reqs, _ in _all_phases(sh, commit, False):
        for r in reqs:
            assert set(r.add) <= kept, "an addend is the kept point of a strictly earlier phase"
            if r.add:
                adds[r.out] = r.add
        kept |= {r.keep for r in reqs if r.keep >= 0}
    expect = {sh.APRIME: (sh.SL_A, sh.SL_CMT1, sh.SL_CMU1), sh.D: (sh.SL_B,)}
    if not commit:
        expect[sh.SL_B] = (sh.SL_A,)
    assert adds == expect
    assert kept == {sh.SL_A, sh.SL_CMT1, sh.SL_CMU1, sh.SL_B} | {sh.TMP(q) for q in range(4)}


def test_gather_lists(sh):
    n = sh.n
    assert sh.basis == list(range(n - 2)) + [sh.G_t, sh.G_u]
    assert sh.gather(sh.GA_NONE, 0) == [] and sh.gather(sh.GA_BASIS, 0) == sh.basis and sh.gather(sh.GA_COL, sh.G_u) == [sh.G_u]
    for j in range(sh.L):
        half = sh.half(j)
        hi, lo = sh.gather(sh.GA_HI, half), sh.gather(sh.GA_LO, half)
        assert hi == sorted(hi) and lo == sorted(lo) and len(hi) == len(lo) == n // 2
        assert sorted(hi + lo) == list(range(n)) and all(k & half for k in hi) and not any(k & half for k in lo)
        assert sh.gather(sh.GA_BASIS_HI, half) == [sh.basis[k] for k in hi]
        assert sh.gather(sh.GA_BASIS_LO, half) == [sh.basis[k] for k in lo]
        assert sh.gather(sh.GA_HI_H, half) == hi + [sh.H] and sh.gather(sh.GA_LO_H, half) == lo + [sh.H]
    assert sh.half(sh.L - 1) == 1


def test_fused_and_split_ipa_rounds_describe_the_same_msm(sh):
    def pairs(r):   # (column, offset of its scalar in the proof's row)
        cols = sh.cols(r.seg0) + sh.cols(r.seg1)
        return Counter((c, r.scal_at + i) for i, c in enumerate(cols))

    for j in range(sh.L):
        split, _ = sh.reqs(IPA, j)
        fused, _ = sh.reqs(IPA_FUSED, j)
        for a, b in zip(split, fused):
            assert a.out == b.out and pairs(a) == pairs(b)
            assert b.seg1.kind == sh.SEG_NONE
