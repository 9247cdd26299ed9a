"""CPU checks of the host-driven prover's transcript and scalar steps (curdleproofs_amd/csrc/host_prove.hpp over host_transcript.hpp), run
in the engine's order by tests/host_emul/host_prove_emul.cpp: once plain and once with -fsanitize=address,undefined.  The group side is
the oracle's.  Every point a step hashes is known up front: the proof points are the oracle's proof bytes, M, the instance rows and H are
compressed by the oracle, D and A' are oracle MSMs as in test_check_weights_cpu.py.  So one run of the twin goes through all steps, and
its outputs are held against the oracle's proof: the serialised bytes, the round vectors folded in Python integers, and the commitments
the staged vectors feed."""
import ctypes
import subprocess

import pytest

from tests.check_harness import build_emul

from tests.test_check_weights_cpu import _slots, emul  # noqa: F401  (emul: host_verify.hpp's twin, the source of D's scalars)

FR, AFF = 32, 96
R_MOD = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
R_INV = pow(1 << 256, -1, R_MOD)      # wire form is the Montgomery residue x * 2^256 mod r
# ell = 4: n = 8, L = 3 — the smallest shape with more than one round, a `half` of 1 in the last round and the n - 2 solved-blinder indices
# next to the vector's start; ell = 28: the README example
SHAPES = [4, 28]
FOUR = ("r_p", "z_k", "z_t", "z_u")


def ints(wire):
    return [int.from_bytes(wire[i:i + FR], "little") * R_INV % R_MOD for i in range(0, len(wire), FR)]


def layout(L):
    """byte offset of every proof point (by slot) and scalar (by name) and the proof's size, written out from CurdleproofsProof::serialize
    (curdleproofs.rs:300-310): the points in slot order, r_p behind C, c and d behind the last R_D, the z's behind cm_B.T_2, x at the end"""
    behind = {14: ["r_p"], 16 + 4 * L: ["c", "d"], 20 + 4 * L: ["z_k", "z_t", "z_u"], 23 + 10 * L: ["x"]}
    off, o = {}, 0
    for slot in range(6, 24 + 10 * L):
        off[slot] = o
        o += 48
        for name in behind.get(slot, []):
            off[name] = o
            o += FR
    return off, o


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def twin(request):
    # (protocol.h, which names the SC_* / V_* scalars, includes hip_runtime.h)
    exe = build_emul("host_prove_emul.cpp", ["host_prove.hpp", "host_transcript.hpp", "host_math.hpp", "prove_reqs.hpp", "layout.hpp", "protocol.h", "mont32.hpp",
                                             "strobe.hpp"], request.param == "sanitized")

    def run(case):
        text = "".join("%s %s\n" % (k, v if isinstance(v, str) else v.hex()) for k, v in case.items())
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout   # a sanitizer report is a non-zero exit
        return {k: bytes.fromhex(v) for k, v in (line.split() for line in out.splitlines())}
    return run


class Case:
    """one oracle instance of `ell` and the twin's input for it"""

    def __init__(self, orc, emul, ell):
        self.orc, self.ell, self.n = orc, ell, ell + 4
        n, L = self.n, (ell + 4).bit_length() - 1
        self.L = L
        self.crs = orc.generate_crs_points(ell)
        self.inst = x = orc.make_instance(ell, 5, self.crs)
        assert x["verdict"] == 1 and len(x["prover_rand"]) == FR * (3 * n + 9)
        self.off, size = layout(L)
        proof = x["proof"]
        assert len(proof) == size
        self.s = s = _slots(L)
        self.nslots = 24 + 10 * L + 2 + 8           # the proof points end at slot 23 + 10 L; D, A', eight scratch slots
        comp = [bytes(48)] * self.nslots
        for slot in range(6, 24 + 10 * L):
            comp[slot] = proof[self.off[slot]:self.off[slot] + 48]
        ic = orc.g1_compress(x["vec_R"] + x["vec_S"] + x["vec_T"] + x["vec_U"])
        mcomp = comp[5] = orc.g1_compress_jac(x["M"])
        self.H = self.crs[AFF * n:AFF * (n + 1)]
        # D = B - beta^-1 sum(G) + alpha sum(H) with the scalars host_verify.hpp derives, A' = A + cm_T.T_1 + cm_U.T_1: oracle MSMs
        points = orc.g1_decompress(b"".join(comp[6:24 + 10 * L]))
        P = lambda slot: points[AFF * (slot - 6):AFF * (slot - 5)]
        g_sum, h_sum = orc.crs_sums(ell, self.crs)
        st, d_scal = emul.cw_new(), ctypes.create_string_buffer(3 * FR)
        try:
            assert emul.cw_prefix(st, ell, L, proof, ic, mcomp, d_scal) == 0
        finally:
            emul.cw_free(st)
        self.slot_D, self.slot_Aprime = 24 + 10 * L, 25 + 10 * L
        comp[self.slot_D] = orc.g1_compress_jac(orc.g1_msm(P(s["B"]) + g_sum + h_sum, d_scal.raw))
        comp[self.slot_Aprime] = orc.g1_compress_jac(orc.g1_msm(P(s["A"]) + P(s["cm_T_T1"]) + P(s["cm_U_T1"]), orc.fr_from_u64(1) * 3))
        self.comp = comp
        self.input = dict(ell=str(ell), perm=" ".join(str(i) for i in x["permutation"]), rand=x["prover_rand"], k=x["k"], m_blinders=x["vec_m_blinders"], ic=ic,
                          mcomp=mcomp, h_comp=orc.g1_compress(self.H), comp=b"".join(comp),
                          final=b"".join(proof[self.off[f]:self.off[f] + FR] for f in ("c", "d", "x")))
        self._out = {}

    def out(self, twin):
        """the twin's outputs for the unchanged instance (one run per build of the twin)"""
        if twin not in self._out:
            self._out[twin] = twin(self.input)
        return self._out[twin]

    def four(self, proof):
        return {f: proof[self.off[f]:self.off[f] + FR] for f in FOUR}

    def rand(self, i, count=1):
        return self.inst["prover_rand"][FR * i:FR * (i + count)]

    def point(self, slot):
        return self.comp[slot]

    def msm(self, bases, scalars):
        return self.orc.g1_compress_jac(self.orc.g1_msm(bases, scalars))


@pytest.fixture(scope="module")
def cases(orc, emul):  # noqa: F811
    return {ell: Case(orc, emul, ell) for ell in SHAPES}


@pytest.mark.parametrize("ell", SHAPES)
def test_serialised_proof_has_the_oracles_scalars_and_every_point_at_its_offset(twin, cases, ell):
    c = cases[ell]
    got, want = c.out(twin)["proof"], c.inst["proof"]
    assert len(got) == len(want)
    assert c.four(got) == c.four(want)           # z_* hang on same_scalar_alpha, and so on every absorb up to it, all IPA rounds included
    for slot in range(6, 24 + 10 * c.L):
        assert got[c.off[slot]:c.off[slot] + 48] == c.point(slot), slot
    assert got == want                           # ... and c, d, x, handed in, at theirs


@pytest.mark.parametrize("ell", SHAPES)
def test_round_vectors_fold_to_the_proofs_c_d_and_x(twin, cases, ell):
    """the fold kernels' rule in Python integers: c_L += gamma^-1 c_R, d_L += gamma d_R, x_L += gamma^-1 x_R"""
    c = cases[ell]
    n, L, o = c.n, c.L, c.out(twin)
    final = {f: int.from_bytes(c.inst["proof"][c.off[f]:c.off[f] + FR], "little") for f in ("c", "d", "x")}
    row, gam = ints(o["ipa_row"]), ints(o["ipa_gamma"])
    assert len(row) == 4 * n and len(gam) == 2 * L
    vc, vd = row[:n], row[n:2 * n]
    assert row[2 * n:3 * n] == [1] * n                         # S_G
    assert row[3 * n:] == ints(o["V_U"])                       # S_G'
    assert ints(o["ipa_beta"]) == [ints(o["sc"])[10]]          # SC_BETA_I
    for j in range(L):
        g, gi, half = gam[2 * j], gam[2 * j + 1], n >> (j + 1)
        assert g * gi % R_MOD == 1
        vc = [(vc[i] + gi * vc[half + i]) % R_MOD for i in range(half)]
        vd = [(vd[i] + g * vd[half + i]) % R_MOD for i in range(half)]
    assert (vc, vd) == ([final["c"]], [final["d"]])
    row, gam = ints(o["smsm_row"]), ints(o["smsm_gamma"])
    assert len(row) == 2 * n and len(gam) == 2 * L
    vx = row[:n]
    assert row[n:] == [1] * n                                  # S_M
    for j in range(L):
        g, gi, half = gam[2 * j], gam[2 * j + 1], n >> (j + 1)
        assert g * gi % R_MOD == 1
        vx = [(vx[i] + gi * vx[half + i]) % R_MOD for i in range(half)]
    assert vx == [final["x"]]


@pytest.mark.parametrize("ell", SHAPES)
def test_staged_vectors_feed_the_commitments_of_the_proof(twin, cases, ell):
    c = cases[ell]
    n, o, s, x = c.n, c.out(twin), c.s, c.inst
    G = c.crs[:AFF * n]                                        # G | Hvec
    assert [len(o[v]) for v in ("V_APERM", "V_C", "V_ZZU", "V_U", "V_D")] == [FR * n] * 5
    assert c.msm(G, o["V_APERM"]) == c.point(s["A"])
    assert c.msm(G, o["V_C"]) == c.point(s["C"])
    assert c.msm(G, o["V_ZZU"]) == c.point(s["B_d"])
    assert c.msm(G, c.rand(6, n)) == c.point(s["B_c"])         # the IR draws
    a, ka, rka = (o["side"][FR * ell * i:FR * ell * (i + 1)] for i in range(3))
    assert a == o["vec_a"]
    assert c.msm(x["vec_R"], a) == c.point(s["R"])
    assert c.msm(x["vec_S"], a) == c.point(s["S"])
    a_perm = o["V_APERM"][:FR * ell]
    assert c.msm(x["vec_R"], ka) == c.msm(x["vec_T"], a_perm)  # k R = sum a_sigma(i) T_i
    assert c.msm(x["vec_S"], ka) == c.msm(x["vec_U"], a_perm)
    # the third row: cm_A.T_2 = r_k R + r_a H, cm_B.T_2 = r_k S + r_b H (same_scalar_argument.rs:60-61)
    assert c.msm(x["vec_R"] + c.H, rka + c.rand(2 * n + 6)) == c.point(s["cm_A_T2"])
    assert c.msm(x["vec_S"] + c.H, rka + c.rand(2 * n + 7)) == c.point(s["cm_B_T2"])


def _with(case, **changed):
    d = dict(case.input)
    d.update(changed)
    return d


def _flip(blob, at):
    return blob[:at] + bytes([blob[at] ^ 1]) + blob[at + 1:]


@pytest.mark.parametrize("ell", SHAPES)
def test_every_input_class_reaches_the_scalars_it_should(twin, orc, cases, ell):
    """one change per input class, and the set of r_p, z_k, z_t, z_u that moves: the challenges up to gprod_alpha reach r_p, every absorb up
    to same_scalar_alpha reaches the z's, the draws RK .. RU reach their own response only.  Two classes cannot move any of the four and
    are pinned by what they do move: a swapped permutation entry (the scalars of A and C, the round vectors), and a byte hashed behind
    same_scalar_alpha (the witness row x for same_msm_step1, the round's gamma for same_msm_loop)."""
    c = cases[ell]
    n, L, s, base = c.n, c.L, c.s, c.out(twin)
    good = c.four(base["proof"])
    ALL, ZS = set(FOUR), {"z_k", "z_t", "z_u"}

    def moved(case_input):
        o = twin(case_input)
        now = c.four(o["proof"])
        return {f for f in FOUR if now[f] != good[f]}, o

    perm = list(c.inst["permutation"])
    perm[0], perm[1] = perm[1], perm[0]
    # (the grand product over all i of a_sigma(i) + sigma(i) alpha + beta is the same for every permutation, and A is hashed as given: a
    # swapped entry moves none of the four, which is the argument's point.  It shows where the permutation is used: in the scalars of A and C)
    got, o = moved(_with(c, perm=" ".join(str(i) for i in perm)))
    assert got == set()
    assert c.msm(c.crs[:AFF * n], o["V_APERM"]) != c.point(s["A"]) and c.msm(c.crs[:AFF * n], o["V_C"]) != c.point(s["C"])
    assert o["ipa_row"][:2 * FR * n] != base["ipa_row"][:2 * FR * n] and o["smsm_row"] != base["smsm_row"]
    other = orc.rng(717).fr(1)
    draws = {"CB": (2, ALL), "RK": (2 * n + 8, {"z_k"}), "RA": (2 * n + 6, {"z_t"}), "RT": (2 * n + 4, {"z_t"}), "RB": (2 * n + 7, {"z_u"}), "RU": (2 * n + 5, {"z_u"})}
    for name, (i, want) in draws.items():
        rand = c.input["rand"]
        assert rand[FR * i:FR * (i + 1)] != other
        assert moved(_with(c, rand=rand[:FR * i] + other + rand[FR * (i + 1):]))[0] == want, name

    point = lambda slot: _with(c, comp=_flip(c.input["comp"], 48 * slot + 47))
    blocks = [("curdleproofs_step1 vec_U", _with(c, ic=_flip(c.input["ic"], 48 * 4 * ell - 1)), ALL),
              ("curdleproofs_step1 M", _with(c, mcomp=_flip(c.input["mcomp"], 47)), ALL),
              ("same_perm_step1 A", point(s["A"]), ALL),
              ("gprod_step1 B", point(s["B"]), ALL),
              ("gprod_step2 C", point(s["C"]), ZS),              # r_p is fixed before C is hashed
              ("ipa_step1 D", point(c.slot_D), ZS),
              ("ipa_step1 B_d", point(s["B_d"]), ZS),
              ("ipa_loop L_C[0]", point(s["L_C"]), ZS),
              ("ipa_loop R_D[L-1]", point(s["R_D"] + L - 1), ZS),
              ("sameexp_points R", point(s["R"]), ZS),
              ("sameexp_points cm_B.T_2", point(s["cm_B_T2"]), ZS)]
    for name, case_input, want in blocks:
        assert moved(case_input)[0] == want, name
    for name, case_input in [("same_msm_step1 A'", point(c.slot_Aprime)), ("same_msm_step1 H", _with(c, h_comp=_flip(c.input["h_comp"], 47))),
                             ("same_msm_step1 B_u", point(s["B_u"]))]:
        got, o = moved(case_input)
        assert got == set() and o["smsm_row"] != base["smsm_row"] and o["ipa_gamma"] == base["ipa_gamma"], name
    for name, slot, j in [("same_msm_loop L_A[0]", s["L_A"], 0), ("same_msm_loop R_U[L-1]", s["R_U"] + L - 1, L - 1)]:
        got, o = moved(point(slot))
        assert got == set() and o["smsm_row"] == base["smsm_row"], name
        first = next(r for r in range(L) if o["smsm_gamma"][2 * FR * r:2 * FR * (r + 1)] != base["smsm_gamma"][2 * FR * r:2 * FR * (r + 1)])
        assert first == j, name
