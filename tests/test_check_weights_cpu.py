"""CPU checks of the verifier's accumulated check (curdleproofs_amd/csrc/check_weights.hpp: the ONE table of weights both verifier paths
apply) and of the host verifier's transcript work (host_verify.hpp), compiled with the host compiler by
tests/host_emul/check_weights_emul.cpp.  The group side — D, A' and the multi-scalar multiplication the GPU would run — is the oracle's:
for a valid proof  sum weight_i . point_i  is the identity, for a proof with one field replaced it is not."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_emul", "check_weights_emul.cpp")
LIB = os.path.join(HERE, "host_emul", "_check_weights.so")
CSRC = os.path.join(HERE, "..", "curdleproofs_amd", "csrc")
FR, AFF = 32, 96
IDENTITY = bytes([0xc0]) + bytes(47)
SHAPES = [28, 60]   # L = 5 and 6: every L-dependent slot offset moves


@pytest.fixture(scope="module")
def emul():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("check_weights.hpp", "host_verify.hpp", "host_math.hpp", "layout.hpp", "mont32.hpp", "strobe.hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.cw_new.restype = vp
    L.cw_free.argtypes = [vp]
    for f in (L.cw_proof_size, L.cw_point_offset, L.cw_scalar_offset):
        f.restype = sz
    L.cw_prefix.argtypes = [vp, sz, sz, vp, vp, vp, vp]
    L.cw_scalars.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, ci, vp, vp, vp]
    L.cw_scalars_fr.argtypes = [vp, sz, sz, vp, ci, vp, vp, vp]
    return L


def _slots(L):
    """slot ids of the proof points by name (layout.hpp SlotMap), written out independently of it"""
    s = {"A": 6, "cm_T_T1": 7, "cm_T_T2": 8, "cm_U_T1": 9, "cm_U_T2": 10, "R": 11, "S": 12, "B": 13, "C": 14, "B_c": 15, "B_d": 16}
    for q, name in enumerate(("L_C", "R_C", "L_D", "R_D")):
        s[name] = 17 + q * L
    at = 17 + 4 * L
    for q, name in enumerate(("cm_A_T1", "cm_A_T2", "cm_B_T1", "cm_B_T2", "B_a", "B_t", "B_u")):
        s[name] = at + q
    for q, name in enumerate(("L_A", "L_T", "L_U", "R_A", "R_T", "R_U")):
        s[name] = at + 7 + q * L
    return s


SCALARS = {"r_p": 0, "c": 1, "d": 2, "z_k": 3, "z_t": 4, "z_u": 5, "x": 6}


class Case:
    """one oracle instance of `ell` with everything about it that does not depend on the proof bytes"""

    def __init__(self, orc, ell):
        self.orc, self.ell, self.n = orc, ell, ell + 4
        self.L = self.n.bit_length() - 1
        self.crs = orc.generate_crs_points(ell)
        self.inst = x = orc.make_instance(ell, 5, self.crs)
        assert x["verdict"] == 1
        self.rows = x["vec_R"] + x["vec_S"] + x["vec_T"] + x["vec_U"]
        self.ic = orc.g1_compress(self.rows)
        self.mcomp = orc.g1_compress_jac(x["M"])
        n = self.n
        pt = lambda i: self.crs[AFF * i:AFF * (i + 1)]
        self.g_sum, self.h_sum = orc.crs_sums(ell, self.crs)
        self.h_comp = orc.g1_compress(pt(n))
        self.crs_bases = self.crs[:AFF * n]                                                          # G | Hvec
        self.singles = pt(n) + pt(n + 1) + pt(n + 2) + self.g_sum + self.h_sum + orc.g1_to_affine(x["M"])   # H G_t G_u G_sum H_sum M
        self.one = orc.fr_from_u64(1)

    def sum(self, emul, proof, factors, both_types=False):
        """(compressed sum weight_i . point_i, the three weight arrays) for `proof`"""
        orc, ell, L, n = self.orc, self.ell, self.L, self.n
        npp, nm = emul.cw_n_points(L), emul.cw_n_slots(L)
        assert len(proof) == emul.cw_proof_size(L)
        points = orc.g1_decompress(b"".join(proof[o:o + 48] for o in (emul.cw_point_offset(L, 6 + q) for q in range(npp))))
        P = lambda slot: points[AFF * (slot - 6):AFF * (slot - 5)]
        st = emul.cw_new()
        try:
            d_scal = ctypes.create_string_buffer(3 * FR)
            assert emul.cw_prefix(st, ell, L, proof, self.ic, self.mcomp, d_scal) == 0
            s = _slots(L)
            d_comp = orc.g1_compress_jac(orc.g1_msm(P(s["B"]) + self.g_sum + self.h_sum, d_scal.raw))
            aprime_comp = orc.g1_compress_jac(orc.g1_msm(P(s["A"]) + P(s["cm_T_T1"]) + P(s["cm_U_T1"]), self.one * 3))
            fused = len(factors) == 12 * FR
            k = [ctypes.create_string_buffer(FR * c) for c in (n, 4 * ell, nm)]
            emul.cw_scalars(st, ell, L, self.ic, self.h_comp, d_comp, aprime_comp, factors, int(fused), *k)
            if both_types:
                kf = [ctypes.create_string_buffer(FR * c) for c in (n, 4 * ell, nm)]
                emul.cw_scalars_fr(st, ell, L, factors, int(fused), *kf)
                assert [b.raw for b in kf] == [b.raw for b in k], "CheckTerms<Fr> and CheckTerms<host::S> differ"
        finally:
            emul.cw_free(st)
        k = [b.raw for b in k]
        total = orc.g1_msm(self.crs_bases + self.rows + self.singles + points, b"".join(k))
        return orc.g1_compress_jac(total), k


@pytest.fixture(scope="module")
def cases(orc):
    return {ell: Case(orc, ell) for ell in SHAPES}


@pytest.mark.parametrize("ell", SHAPES)
@pytest.mark.parametrize("nfactors", [8, 12], ids=["per_proof_factors", "fused_factors"])
def test_valid_proof_sums_to_the_identity_with_every_weight_present_on_both_scalar_types(emul, orc, cases, ell, nfactors):
    c = cases[ell]
    factors = c.inst["verifier_rand"] if nfactors == 8 else orc.rng(31 + ell).fr(12)
    total, k = c.sum(emul, c.inst["proof"], factors, both_types=True)
    assert total == IDENTITY
    nm = emul.cw_n_slots(c.L)
    assert nm == 6 + emul.cw_n_points(c.L) == 6 + 18 + 10 * c.L
    assert [len(x) // FR for x in k] == [c.n, 4 * ell, nm]
    weights = b"".join(k)
    zero = [i for i in range(len(weights) // FR) if weights[FR * i:FR * (i + 1)] == bytes(FR)]
    assert zero == [], "points without a weight"


def _mutations(L):
    """the 17 single-field mutations of test_single_field_negatives_of_every_sub_argument (tests/test_gpu_parity.py), then z_t and z_u"""
    return [("r_p", 0), ("c", 0), ("d", 0), ("x", 0), ("z_k", 0), ("A", 0), ("cm_T_T1", 0), ("R", 0), ("B", 0), ("C", 0), ("B_c", 0), ("L_C", 1),
            ("R_D", 0), ("cm_A_T2", 0), ("B_a", 0), ("L_T", 0), ("R_U", L - 1), ("z_t", 0), ("z_u", 0)]


@pytest.mark.parametrize("ell", SHAPES)
@pytest.mark.parametrize("nfactors", [8, 12], ids=["per_proof_factors", "fused_factors"])
def test_every_mutated_proof_is_caught(emul, orc, cases, ell, nfactors):
    c = cases[ell]
    x, good = c.inst, c.inst["proof"]
    factors = x["verifier_rand"] if nfactors == 8 else orc.rng(31 + ell).fr(12)
    rng = orc.rng(717)
    scalar = orc.fr_to_canonical_bytes(rng.fr(1))
    point = orc.g1_compress(rng.g1_affine(1))
    slots = _slots(c.L)
    assert len(_mutations(c.L)) == 19
    for field, j in _mutations(c.L):
        if field in SCALARS:
            o, repl = emul.cw_scalar_offset(c.L, SCALARS[field]), scalar
        else:
            o, repl = emul.cw_point_offset(c.L, slots[field] + j), point
        assert good[o:o + len(repl)] != repl
        bad = good[:o] + repl + good[o + len(repl):]
        assert orc.verify(ell, c.crs, x["vec_R"], x["vec_S"], x["vec_T"], x["vec_U"], x["M"], bad, x["verifier_rand"]) == 0, field
        total, _ = c.sum(emul, bad, factors)
        assert total != IDENTITY, field
