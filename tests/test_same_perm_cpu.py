"""CPU side of cpx_same_perm_prove / cpx_same_perm_verify: the oracle shim (tests/same_perm_lib.py) pinned to the oracle's verifier and to
the grand-product shim of tests/gprod_lib.py; same_perm_plan.hpp and same_perm_algebra.hpp compiled for the CPU
(tests/host_emul/same_perm_plan_emul.cpp, plain and as a stand-alone sanitized program) against Python integers; the extra relation's weights
on the oracle's own points; step 1 of the transcript on tests/strobe_ref.py with the entry states the GPU test uses; the new names in the
header, EXPORTS, the Rust source and the library."""
import functools
import os
import re
import subprocess

import pytest

from tests import gprod_lib as gl, same_perm_lib as sl, strobe_ref, subarg_lib, subarg_verify_lib as sv
from tests.check_harness import build_emul
from tests.subarg_lib import IPA, R_

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FR, AFF, JAC = 32, 96, 144
NAMES = ("cpx_same_perm_prove", "cpx_same_perm_prove_rng", "cpx_same_perm_verify")
T = sl.THREADS
HEXKEYS = ("factors", "product", "serial", "vproduct", "vserial", "rb", "bsc", "w")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    deps = ["same_perm_plan.hpp", "same_perm_algebra.hpp", "gprod_plan.hpp", "gprod_algebra.hpp", "subarg_check_plan.hpp", "subarg_prove_plan.hpp", "loop_plan.hpp",
            "tier0_plan.hpp", "mont32.hpp"]
    exe = build_emul("same_perm_plan_emul.cpp", deps, request.param == "sanitized", hip=False)   # sanitized: a program with its own main, run as such

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout       # a sanitizer report is a non-zero exit
        res = {}
        for line in out.splitlines():
            key, *vals = line.split()
            vals = [int(v, 16) for v in vals] if key in HEXKEYS else [int(v) for v in vals]
            res[key] = vals
        return res

    return run


def _ints(orc, seed, k):
    return subarg_lib.to_ints(orc, orc.rng(seed).fr(k)) if k else []


def _hex(v):
    return "%x" % (v % R_)


# ---- the shim ----
@pytest.fixture(scope="module")
def pinned(orc):
    ell, nb = 12, 4
    c = sl.sp_inputs(11, ell, nb, filler=b"pinned")
    d = sl.seeded_draws(orc, 12, ell, nb)
    return c, d, sl.sp_prove(c, d)


def test_shim_proves_and_its_verifier_accepts(orc, pinned):
    c, d, w = pinned
    v = sl.sp_verify(c, w["proof"], sl.factors(orc, 13))
    assert w["ok"] and v["verdict"] is True and v["state"] == w["state"]           # prover and verifier leave the same transcript
    assert len(w["proof"]) == sl.proof_bytes(4) and len(w["challenges"]) == sl.n_challenges(4) * FR
    other = sl.sp_inputs(14, 12, 4, filler=b"pinned")
    assert sl.sp_verify(dict(c, A=other["A"]), w["proof"], sl.factors(orc, 13))["verdict"] is False
    assert sl.sp_verify(dict(c, a=other["a"]), w["proof"], sl.factors(orc, 13))["verdict"] is False


def test_shim_is_pinned_to_the_grand_product_shim(orc, pinned):
    """sp_gprod from the state of a filler gives gprod_oracle.cpp's gp_prove bytes; from the state after step 1, on the B, result, factors and
    blinders sp_derive exports, it gives the bytes sp_prove embeds behind B — and gp_prove's own C, which hangs on no transcript"""
    c, d, w = pinned
    g = gl.gp_inputs(21, 12, 4, filler=b"abc")
    gd = gl.seeded_draws(orc, 22, 12, 4)
    want = gl.gp_prove(g, gd)
    got = sl.sp_gprod(g, g["state_in"], g["B"], g["result"], g["b"], g["rb"], gd)
    assert want["ok"] and got["proof"] == want["proof"] and got["state"] == want["state"]
    dv = sl.sp_derive(c)
    emb = sl.sp_gprod(c, dv["state"], dv["B"], dv["result"], dv["b"], dv["rb"], d)
    assert w["proof"][:48] == orc.g1_compress_jac(dv["B"])
    assert w["proof"][48:] == emb["proof"] and w["state"] == emb["state"]
    assert w["challenges"][:2 * FR] == dv["alpha"] + dv["beta"]
    same = gl.gp_prove(dict(g, G=c["G"], H=c["H"], crs_U=c["crs_U"], B=dv["B"], result=dv["result"], b=dv["b"], rb=dv["rb"]), d)
    assert same["proof"][:48] == emb["proof"][:48]                                 # C = <vec_c, G> + <vec_c_blinders, H>
    ai, p = subarg_lib.to_ints(orc, c["a"]), sl.perm_list(c["perm"])
    alpha, beta = subarg_lib.to_ints(orc, dv["alpha"] + dv["beta"])
    f = sl.model_factors(ai, p, alpha, beta)
    assert subarg_lib.to_ints(orc, dv["b"]) == f
    prod = functools.reduce(lambda x, y: x * y % R_, f, 1)
    assert subarg_lib.to_ints(orc, dv["result"]) == [prod]
    ra, rm = subarg_lib.to_ints(orc, c["ra"]), subarg_lib.to_ints(orc, c["rm"])
    assert subarg_lib.to_ints(orc, dv["rb"]) == [(x + alpha * y) % R_ for x, y in zip(ra, rm)]


def test_shim_says_where_the_reference_panics(orc):
    c = sl.sp_inputs(31, 2, 2)
    d = sl.seeded_draws(orc, 32, 2, 2)
    w = sl.sp_prove(c, bytes(FR) + d[FR:])                                        # vec_c_blinders[0] = c[n - 2] = 0
    assert not w["ok"] and w["proof"] == bytes(sl.proof_bytes(2)) and w["state"] == c["state_in"]
    assert sl.sp_prove(c, d)["ok"]


# ---- the algebra ----
@pytest.mark.parametrize("ell,nb,workers", [(1, 1, T), (3, 1, T), (6, 2, 4), (T - 1, 1, T), (T, 0, T), (T + 1, 3, T), (2 * T + 5, 3, T), (252, 4, T), (60, 4, 7)])
def test_layer_matches_the_integer_model(emul, orc, ell, nb, workers):
    alpha, beta = _ints(orc, 400 + ell, 2)
    a, ra, rm = _ints(orc, 401 + ell, ell), _ints(orc, 402 + ell, nb), _ints(orc, 403 + ell, nb)
    perm = [(7 * i + 3) % ell for i in range(ell)] if ell % 7 else list(range(ell))[::-1]
    if ell > 2:
        perm[1] = perm[0]                                                         # a repeated entry is legal
    out = emul("layer", workers, ell, nb, _hex(alpha), _hex(beta), *map(_hex, a), *["%x" % s for s in perm], *map(_hex, ra), *map(_hex, rm))
    f = sl.model_factors(a, perm, alpha, beta)
    mul = lambda v: functools.reduce(lambda x, y: x * y % R_, v, 1)
    assert out["factors"] == f
    assert out["product"] == out["serial"] == [mul(f)]
    assert out["vproduct"] == out["vserial"] == [mul(sl.model_factors(a, range(ell), alpha, beta))]
    assert out.get("rb", []) == [(x + alpha * y) % R_ for x, y in zip(ra, rm)]
    assert out["bsc"] == [beta] * ell + [alpha]


def test_product_with_a_zero_factor(emul, orc):
    ell, alpha, beta = 9, 5, 11
    a = _ints(orc, 450, ell)
    perm = list(range(ell))
    a[4] = -(4 * alpha + beta) % R_
    out = emul("layer", T, ell, 0, _hex(alpha), _hex(beta), *map(_hex, a), *["%x" % s for s in perm])
    assert out["factors"][4] == 0 and out["product"] == [0] and out["vproduct"] == [0]


def test_canonical_words_are_the_little_endian_scalar(emul):
    for v in (0, 1, R_ - 1, 0x0123456789abcdef << 64):
        assert emul("canon", _hex(v))["words"] == [(v >> (32 * j)) & 0xffffffff for j in range(8)]


def test_weights_match_the_integer_model(emul, orc):
    a0, alpha, beta = _ints(orc, 460, 3)
    m = sl.model_weights(a0, alpha, beta)
    assert emul("weights", _hex(a0), _hex(alpha), _hex(beta))["w"] == [m["g_add"], m["B"], m["A"], m["M"]]


# ---- the plans ----
def _regions(out, prefix):
    return sorted((v[0], v[1], k) for k, v in out.items() if k.startswith(prefix + "."))


@pytest.mark.parametrize("count,ell,nb", [(1, 1, 1), (3, 6, 2), (2, 8, 0), (5, 124, 4), (1, 4092, 4)])
def test_prover_plan_regions_do_not_overlap_and_the_proof_byte_order(emul, count, ell, nb):
    out = emul("plan", count, ell, nb)
    L = sl.log2(ell + nb)
    assert out["status"] == [0]
    end = {}
    for kind in ("fr", "ix", "jac", "aff", "by", "task"):
        at = 0
        for start, size, name in _regions(out, kind):
            assert start == at, (kind, name)                                      # back to back, the grand-product plan's total first
            at = start + size
        end[kind] = at
    sizes = {k: v[1] for k, v in out.items() if "." in k}
    # the totals the engine reserves by are the end of the last region of every kind: this layer's, the grand-product layer's below it
    # (the layer raises no flag and its B sums land in the grand-product layer's B slots: those two ends are the layer's below)
    flags, res = out["flags_total"][0], max(out["res_end"])
    assert out["totals"][:8] == [end["fr"], end["jac"], end["aff"], end["by"], flags, end["ix"], end["task"], res]
    assert out["totals_gp"][:8] == [sizes["fr.gp"], sizes["jac.gp"], sizes["aff.gp"], sizes["by.gp"], flags, sizes["ix.gp"], sizes["task.gp"], res]
    assert flags == 2 * count and out["res_end"] == [2 * count, L * count * 4] and out["totals_core"][4] == count and out["totals_core"][7] == L * count * 4
    # ... and what leads the inner-product proof's bytes and challenges at the three depths
    assert [out[k][8:] for k in ("totals_core", "totals_gp", "totals")] == [[0, 0], [80, 2], [128, 4]]
    assert sizes["fr.a"] == count * ell and sizes["fr.ra"] == sizes["fr.rm"] == count * nb and sizes["fr.bsc"] == count * (ell + 1) and sizes["fr.chal"] == 2 * count
    assert sizes["ix.perm"] == count * ell and sizes["ix.gather"] == ell + 1 and sizes["ix.addend"] == count
    assert sizes["jac.A"] == sizes["jac.M"] == sizes["aff.A"] == sizes["aff.M"] == sizes["task.B"] == count and sizes["by.A"] == sizes["by.M"] == 48 * count
    assert out["bytes"] == [0, 48, 96, 128]                                       # B | C | r_p | the InnerProductProof (:173-177, grand_product_argument.rs:248-253)
    assert out["proof_bytes"] == [sl.proof_bytes(L)] == [48 * (4 + 4 * L) + 96]
    assert out["challenges"] == [6 + L] and out["draws_each"] == [gl.draws_each(ell, nb)] and out["message_bytes"] == [8 + 32 * ell]
    stride, h = out["row"]
    n = ell + nb
    assert stride == 2 * n + 1 and h == 2 * n                                     # M sits in the row's H slot, outside G | H and their copy
    assert out["gather"] == list(range(ell)) + [h]
    assert out["addend"] == [out["aff.A"][0] + i - out["aff_B"][0] for i in range(count)]
    assert out["msm"] == [1, count, count * (ell + 1), ell + 1]


@pytest.mark.parametrize("count,ell,nb", [(1, 1, 0), (1, 1, 1), (3, 6, 2), (2, 8, 0), (5, 124, 4)])
def test_verifier_plan_regions_do_not_overlap_and_the_row_grows_by_three(emul, count, ell, nb):
    out = emul("check", count, ell, nb)
    n = ell + nb
    L = sl.log2(n)
    assert out["status"] == [0]
    end = {}
    for kind in ("fr", "by", "st", "ix", "jac"):
        at = 0
        for start, size, name in _regions(out, kind):
            assert start == at, (kind, name)
            at = start + size
        end[kind] = at
    # the totals the engine reserves by are the end of the last region of every kind (the dense affine points are the grand-product
    # layer's; one task and one sum per item) ...
    sizes = {k: v[1] for k, v in out.items() if "." in k}
    aff = out["aff_total"][0]
    assert out["totals"][:8] == [end["fr"], end["jac"], aff, end["by"], end["st"], end["ix"], count, count] and aff == 5 * count
    assert out["totals_gp"][:8] == [sizes["fr.gp"], sizes["jac.stmt"], aff, sizes["by.gp"], sizes["st.gp"], sizes["ix.gp"], count, count]
    assert out["totals_core"][1:3] == [3 * count, 0] and out["totals_core"][4] == sizes["st.gp"] - 2 * count
    # ... and what leads the inner-product proof's bytes and challenges at the three depths
    assert [out[k][8:] for k in ("totals_core", "totals_gp", "totals")] == [[0, 0], [80, 2], [128, 4]]
    assert out["checks"] == [3] and out["challenges"] == [6 + L] and out["proof_bytes"] == [sl.proof_bytes(L)]
    inner = n + 4 * L + 5                                                         # the inner-product check's row (subarg_check_plan.hpp)
    assert out["points"] == [inner + 3] and out["row"] == [inner - 3, inner, inner + 1, inner + 2]
    assert out["fr_weights_end"] == [count * (inner + 3)]                         # the weights of the longer rows are what the check's other regions follow
    assert out["lists"] == [i * (inner + 3) + inner + 1 for i in range(count)] + [i * (inner + 3) + inner + 2 for i in range(count)]


def test_plans_refuse_what_the_grand_product_plans_refuse(emul):
    assert emul("plan", 1, 0, 4)["status"] == [gl_status("GPROD_NO_FACTOR")]
    assert emul("plan", 1, 1, 0)["status"] == [gl_status("GPROD_NO_BLINDERS")]
    assert emul("plan", 1, 3, 0)["status"] == [gl_status("GPROD_NOT_POW2")]
    assert emul("plan", 16385, 2, 2)["status"] == [gl_status("GPROD_TOO_LARGE")]
    assert emul("check", 1, 3, 0)["status"] == [1] and emul("check", 65537, 2, 2)["status"] == [2]
    big = (1 << 24) // (256 + 4 * 8 + 5 + 3)                                      # count (n + 4 L + 8) <= 2^24: the three further points count
    assert big + 1 <= (1 << 24) // (256 + 4 * 8 + 5) and big < 65536
    assert emul("check", big, 252, 4)["status"] == [0] and emul("check", big + 1, 252, 4)["status"] == [2]


def gl_status(name):
    return ("GPROD_OK", "GPROD_NOT_POW2", "GPROD_TOO_LARGE", "GPROD_NO_FACTOR", "GPROD_NO_BLINDERS").index(name)


# ---- the extra relation's weights on the oracle's points ----
def _row(orc, c, proof, f3, chal):
    """the item's row of points and of weights as same_perm_plan.hpp lays them out: G | H, the inner-product proof's points, crs_U, C, D,
    then B, A, M.  The weights come from the integer models; points are the oracle's.  Returns (points affine wire, weights ints)."""
    ell, nb = c["ell"], c["nb"]
    n = ell + nb
    L = sl.log2(n)
    ci = subarg_lib.to_ints(orc, chal)
    sa, sb, ga, gb = ci[:4]
    a = subarg_lib.to_ints(orc, f3)
    HEAD = 128
    r_p = int.from_bytes(proof[96:128], "little")
    ai = subarg_lib.to_ints(orc, c["a"])
    result = functools.reduce(lambda x, y: x * y % R_, sl.model_factors(ai, range(ell), sa, sb), 1)
    gbi = pow(gb, R_ - 2, R_)
    u = [pow(gbi, i + 1, R_) for i in range(ell)] + [pow(gbi, ell + 1, R_)] * nb
    inner = (r_p * pow(gb, ell + 1, R_) + result * pow(gb, ell, R_) - 1) % R_
    fin = [int.from_bytes(proof[-64:-32], "little"), int.from_bytes(proof[-32:], "little")]
    w = sv.model_row(IPA, n, a[1:], ci[4:], fin, z=inner, u=u)
    m = sl.model_weights(a[0], sa, sb)
    w = [(x + m["g_add"]) % R_ for x in w[:ell]] + w[ell:] + [m["B"], m["A"], m["M"]]
    B = orc.g1_decompress(proof[:48])
    C = orc.g1_decompress(proof[48:96])
    D = orc.g1_to_affine(orc.g1_msm(B + c["g_sum"] + c["h_sum"], subarg_lib.to_wire(orc, [1, -gbi, ga])))
    pts = c["G"] + c["H"] + b"".join(orc.g1_decompress(proof[HEAD + 48 * s:HEAD + 48 * (s + 1)]) for s in range(2 + 4 * L))
    pts += orc.g1_to_affine(c["crs_U"]) + C + D + B + orc.g1_to_affine(c["A"]) + orc.g1_to_affine(c["M"])
    assert len(pts) == len(w) * AFF == (n + 4 * L + 8) * AFF
    return pts, w


def _vanishes(orc, pts, w):
    return orc.g1_to_affine(orc.g1_msm(pts, subarg_lib.to_wire(orc, w))) == bytes(AFF)


def test_row_vanishes_for_an_honest_item_and_for_no_broken_one(orc):
    """the flattened check on the oracle's points.  Honest: the weighted sum is the identity.  B shifted by a multiple of an H base while the
    grand-product relations still hold: the sum with a_0 = 0 (the grand-product relations alone) still vanishes, the whole sum does not.
    A flipped r_p: the same-permutation part alone (a_1 = a_2 = 0) vanishes, the whole sum does not."""
    ell, nb = 6, 2
    c = sl.sp_inputs(8400, ell, nb)
    d = sl.seeded_draws(orc, 8401, ell, nb)
    f3 = sl.factors(orc, 8402)
    only0, only12 = f3[:FR] + bytes(2 * FR), bytes(FR) + f3[FR:]
    w = sl.sp_prove(c, d)
    assert sl.sp_verify(c, w["proof"], f3)["verdict"] is True
    assert _vanishes(orc, *_row(orc, c, w["proof"], f3, w["challenges"]))
    # only the same-permutation relation broken
    dv = sl.sp_derive(c)
    rb = subarg_lib.to_ints(orc, dv["rb"])
    rb2 = subarg_lib.to_wire(orc, [rb[0] + 5] + rb[1:])
    B2 = orc.g1_msm(c["G"] + c["H"], dv["b"] + rb2)
    g = sl.sp_gprod(c, dv["state"], B2, dv["result"], dv["b"], rb2, d)
    proof2 = orc.g1_compress_jac(B2) + g["proof"]
    assert sl.sp_verify(c, proof2, f3)["verdict"] is False
    chal2 = _challenges_of(orc, c, proof2)
    assert not _vanishes(orc, *_row(orc, c, proof2, f3, chal2))
    assert _vanishes(orc, *_row(orc, c, proof2, only12, chal2))
    assert not _vanishes(orc, *_row(orc, c, proof2, only0, chal2))
    # only a grand-product relation broken
    proof3 = w["proof"][:96] + bytes([w["proof"][96] ^ 1]) + w["proof"][97:]
    assert sl.sp_verify(c, proof3, f3)["verdict"] is False
    chal3 = _challenges_of(orc, c, proof3)
    assert not _vanishes(orc, *_row(orc, c, proof3, f3, chal3))
    assert _vanishes(orc, *_row(orc, c, proof3, only0, chal3))


def _challenges_of(orc, c, proof):
    """the verifier's challenges for given proof bytes, on tests/strobe_ref.py: same-perm alpha, beta, gprod alpha, beta, ipa alpha, beta, gammas"""
    ell, nb = c["ell"], c["nb"]
    L = sl.log2(ell + nb)
    ai = subarg_lib.to_ints(orc, c["a"])
    t, sa, sb = sl.model_step1(c["state_in"], orc.g1_compress_jac(c["A"]), orc.g1_compress_jac(c["M"]), ai)
    result = functools.reduce(lambda x, y: x * y % R_, sl.model_factors(ai, range(ell), sa, sb), 1)
    r_p = int.from_bytes(proof[96:128], "little")
    t.append_message(b"gprod_step1", proof[:48])
    t.append_scalar(b"gprod_step1", result)
    ga = t.get_and_append_challenge(b"gprod_alpha")[0]
    t.append_message(b"gprod_step2", proof[48:96])
    t.append_scalar(b"gprod_step2", r_p)
    gb = t.get_and_append_challenge(b"gprod_beta")[0]
    gbi = pow(gb, R_ - 2, R_)
    B = orc.g1_decompress(proof[:48])
    D = orc.g1_msm(B + c["g_sum"] + c["h_sum"], subarg_lib.to_wire(orc, [1, -gbi, ga]))
    inner = (r_p * pow(gb, ell + 1, R_) + result * pow(gb, ell, R_) - 1) % R_
    pt = lambda s: proof[128 + 48 * s:128 + 48 * (s + 1)]
    t.append_message(b"ipa_step1", proof[48:96])
    t.append_message(b"ipa_step1", orc.g1_compress_jac(D))
    t.append_scalar(b"ipa_step1", inner)
    t.append_message(b"ipa_step1", pt(0))
    t.append_message(b"ipa_step1", pt(1))
    out = [sa, sb, ga, gb, t.get_and_append_challenge(b"ipa_alpha")[0], t.get_and_append_challenge(b"ipa_beta")[0]]
    for j in range(L):
        for name in ("L_C", "L_D", "R_C", "R_D"):
            t.append_message(b"ipa_loop", pt(sv.slot(IPA, L, name, j)))
        out.append(t.get_and_append_challenge(b"ipa_gamma")[0])
    return subarg_lib.to_wire(orc, out)


def test_challenge_model_is_the_oracles(orc, pinned):
    c, d, w = pinned
    assert _challenges_of(orc, c, w["proof"]) == w["challenges"]


# ---- step 1 on the reference transcript ----
SHAPES = ((3, 1), (7, 1))


def _step1_events(ell, f):
    """where step 1 from the state of an f-byte filler puts the vec_a message and the next operation header: (pos, length, header pos)"""
    t, _, _ = sl.model_step1(subarg_lib.entry_state(bytes(f)), bytes(48), bytes(48), [0] * ell)
    tr = t.trace
    at = next(i for i, e in enumerate(tr) if e[0] == "bytes" and e[1] == "data" and e[3] == 8 + 32 * ell)
    header = next(e[1] for e in tr[at + 1:] if e[0] == "header")
    return tr[at][2], tr[at][3], header


def _crossings(ell, f):
    pos, size, header = _step1_events(ell, f)
    cuts = [x for x in range(1, size) if (pos + x) % strobe_ref.RATE == 0]       # the message bytes ahead of every boundary inside it
    out = set()
    if any(x < 8 for x in cuts):
        out.add("prefix")
    if any(8 + 32 <= x < size - 32 and (x - 8) % 32 for x in cuts):
        out.add("scalar")                                                         # a scalar that is neither the first nor the last, cut inside
    if size - 1 in cuts:
        out.add("last_byte")                                                      # the boundary falls ahead of the message's last byte
    if (pos + size) % strobe_ref.RATE == 0:
        out.add("ends_on_boundary")
    if header == strobe_ref.RATE - 1:
        out.add("header")                                                         # the two header bytes of the challenge's first operation are cut apart
    return out


@functools.lru_cache(maxsize=None)
def boundary_cases():
    """per crossing the first (ell, n_blinders, filler length) that shows it: ((name, ell, nb, f), ...), searched on tests/strobe_ref.py (the
    positions do not depend on the values absorbed)"""
    wanted = ["prefix", "scalar", "last_byte", "header", "ends_on_boundary"]
    found = {}
    for ell, nb in SHAPES:
        for f in range(1, 2 * strobe_ref.RATE):
            for name in _crossings(ell, f):
                found.setdefault(name, (name, ell, nb, f))
            if len(found) == len(wanted):
                return tuple(found[k] for k in wanted)
    return tuple(found[k] for k in wanted if k in found)


def test_step_1_against_the_reference_transcript_at_every_crossing(orc):
    cases = boundary_cases()
    assert [name for name, _, _, _ in cases] == ["prefix", "scalar", "last_byte", "header", "ends_on_boundary"]
    for name, ell, nb, f in cases:
        assert name in _crossings(ell, f)
        c = sl.sp_inputs(680 + f, ell, nb, filler=bytes(f))
        dv = sl.sp_derive(c)                                                      # the oracle's Merlin
        t, alpha, beta = sl.model_step1(c["state_in"], orc.g1_compress_jac(c["A"]), orc.g1_compress_jac(c["M"]), subarg_lib.to_ints(orc, c["a"]))
        assert subarg_lib.to_ints(orc, dv["alpha"] + dv["beta"]) == [alpha, beta], name
        assert subarg_lib.state_bytes(t.to_words()) == dv["state"], name
        pos, size, _ = _step1_events(ell, f)
        assert size == 8 + 32 * ell


def test_one_message_not_a_list_of_scalars():
    """vec_a is ONE message (its length, then the scalars): ell appends of 32 bytes leave another state"""
    st = subarg_lib.entry_state(b"x")
    a = [5, 6, 7]
    t, _, _ = sl.model_step1(st, bytes(48), bytes(48), a)
    u = strobe_ref.Transcript.from_words(subarg_lib.words(st))
    u.append_message(b"same_perm_step1", bytes(48))
    u.append_message(b"same_perm_step1", bytes(48))
    for x in a:
        u.append_scalar(b"same_perm_step1", x)
    u.get_and_append_challenge(b"same_perm_alpha")
    u.get_and_append_challenge(b"same_perm_beta")
    assert t.to_words() != u.to_words()
    assert sl.vec_a_message(a)[:8] == (3).to_bytes(8, "little") and len(sl.vec_a_message(a)) == 8 + 96


# ---- names ----
def test_names_agree_in_header_exports_and_library():
    import curdleproofs_amd as cpx
    header = open(os.path.join(ROOT, "include", "cpx.h")).read()
    rust = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header) and re.search(r"pub fn %s\(" % name, rust)
        assert name in cpx.EXPORTS
    lib = os.path.join(ROOT, "curdleproofs_amd", "_lib", "libcpx.so")
    if os.path.exists(lib):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
        for name in NAMES:
            assert re.search(r" T %s$" % name, syms, re.M)
    for k in ("k_same_perm_step", "k_same_perm_verify_step", "k_same_perm_weights"):
        assert k in cpx.Context.KERNELS
    assert callable(cpx.Context.same_perm_prove) and callable(cpx.Context.same_perm_verify)
    for cite in ("same_permutation_argument.rs:40-99", "same_permutation_argument.rs:112-171", ":173-177", ":149", "util.rs:78"):
        assert cite in header
    assert sl.PIECE == int(re.search(r"SAME_PERM_PIECE = (\d+)", open(os.path.join(ROOT, "curdleproofs_amd", "csrc", "same_perm_plan.hpp")).read()).group(1))
    for src in ("build.py",):
        assert "same_perm.hip" in open(os.path.join(ROOT, "curdleproofs_amd", src)).read()
    assert "same_perm.hip" in open(os.path.join(ROOT, "scripts", "sanitize_engine.sh")).read()
