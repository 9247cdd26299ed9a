"""CPU side of cpx_gprod_prove: the oracle shim (tests/gprod_lib.py) pinned to the oracle's verifier and to the inner-product shim of
tests/subarg_prove_lib.py; gprod_algebra.hpp compiled for the CPU (tests/host_emul/gprod_plan_emul.cpp, plain and sanitized) against
Python integers; gprod_plan.hpp against a Python model of the layout; the model of steps 1 and 2 the GPU test searches entry states
with against the oracle; the new names in the header, EXPORTS, the Rust source and the library."""
import os
import re
import subprocess

import pytest

from tests import gprod_lib as gl, subarg_lib, subarg_prove_lib as sp, subarg_verify_lib as sv
from tests.check_harness import build_emul
from tests.subarg_lib import IPA, R_

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FR, AFF, JAC = 32, 96, 144
NAMES = ("cpx_gprod_prove", "cpx_gprod_prove_rng", "cpx_gprod_verify")
T = gl.THREADS


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    deps = ["gprod_plan.hpp", "gprod_algebra.hpp", "subarg_check_plan.hpp", "subarg_prove_plan.hpp", "loop_plan.hpp", "tier0_plan.hpp", "mont32.hpp", "modinv30.hpp"]
    exe = build_emul("gprod_plan_emul.cpp", deps, request.param == "sanitized", hip=False)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout       # a sanitizer report is a non-zero exit
        res = {}
        for line in out.splitlines():
            key, *vals = line.split()
            vals = [int(v, 16) for v in vals] if key in ("c", "u", "uv", "d", "dsc", "r_p", "inner_prod") else [int(v) for v in vals]
            res[key] = vals[0] if len(vals) == 1 and key not in ("c", "u", "uv", "d", "dsc", "addend", "lists") else vals
        return res

    return run


def _ints(orc, seed, k):
    return subarg_lib.to_ints(orc, orc.rng(seed).fr(k)) if k else []


# ---- the shim ----
@pytest.fixture(scope="module")
def pinned(orc):
    ell, nb = 124, 4
    c = gl.gp_inputs(11, ell, nb)
    d = gl.seeded_draws(orc, 12, ell, nb)
    return c, d, gl.gp_prove(c, d)


def test_shim_proves_and_its_verifier_accepts(orc, pinned):
    c, d, w = pinned
    f = sv.factors(orc, 13, IPA)
    v = gl.gp_verify(c, w["proof"], f)
    assert w["ok"] and v["verdict"] is True and v["state"] == w["state"]           # prover and verifier leave the same transcript
    assert len(w["proof"]) == gl.proof_bytes(7) and len(w["challenges"]) == gl.n_challenges(7) * FR


def test_shim_rejects_another_result_and_a_scaled_B(orc, pinned):
    """grand_product_argument.rs:330-366: gprod_result + 1 and B * s do not verify"""
    c, d, w = pinned
    f = sv.factors(orc, 13, IPA)
    plus_one = subarg_lib.to_wire(orc, [subarg_lib.to_ints(orc, c["result"])[0] + 1])
    assert gl.gp_verify(dict(c, result=plus_one), w["proof"], f)["verdict"] is False
    s = orc.rng(14).fr(1)
    scaled = orc.g1_msm(orc.g1_to_affine(c["B"]), s)
    assert not orc.g1_eq_jac(scaled, c["B"])
    assert gl.gp_verify(dict(c, B=scaled), w["proof"], f)["verdict"] is False
    assert gl.gp_verify(dict(c, g_sum=c["h_sum"]), w["proof"], f)["verdict"] is False                # the sums are taken from the caller
    assert gl.gp_verify(c, w["proof"][:48] + bytes([0xff] * 32) + w["proof"][80:], f)["verdict"] == "deserialize"   # r_p >= r


def test_shim_hands_the_inner_product_prover_what_the_reference_does(orc, pinned):
    """the whole embedded IPA byte string is what the oracle's ipa_new gives on the derived (G | H, G', C, D, inner_prod, c, d) from the
    state after step 2 with the same draws (gp_inner), and the two end in the same state.  sp_prove of
    tests/host_emul/subarg_prove_oracle.cpp on the same derived inputs starts from a fresh transcript, so of its bytes B_c and B_d,
    which no challenge enters, are compared; the derived statement is one the witness satisfies."""
    c, d, w = pinned
    nb, n = c["nb"], c["ell"] + c["nb"]
    dv = gl.gp_derive(c, d[:nb * FR])
    own = gl.gp_inner(c, d)
    assert own["proof"] == w["proof"][80:] and own["state"] == w["state"]
    item = dict(kind=IPA, n=n, filler=b"", bases=dv["bases"], stmt=dv["stmt"], z=dv["z"], vecs=dv["vecs"])
    inner = sp.sp_prove(item, d[nb * FR:])
    assert inner["ok"] and inner["proof"][:96] == w["proof"][80:176]
    assert orc.g1_compress_jac(dv["stmt"][1]) == w["proof"][:48]
    ints = lambda x: subarg_lib.to_ints(orc, x)
    assert sum(a * b for a, b in zip(ints(dv["vecs"][0]), ints(dv["vecs"][1]))) % R_ == ints(dv["z"])[0]
    assert orc.g1_eq_jac(orc.g1_msm(dv["bases"][0], dv["vecs"][0]), dv["stmt"][1]) and orc.g1_eq_jac(orc.g1_msm(dv["bases"][1], dv["vecs"][1]), dv["stmt"][2])
    alpha, beta = ints(w["challenges"][:2 * FR])
    m = gl.model_layer(ints(c["b"]), ints(c["rb"]), ints(d[:nb * FR]), ints(c["result"])[0], alpha, beta)
    assert ints(dv["vecs"][1]) == m["d"] and ints(dv["z"])[0] == m["inner_prod"] and ints(dv["vecs"][0]) == gl.model_products(ints(c["b"])) + ints(d[:nb * FR])
    assert orc.g1_scale(dv["bases"][0], subarg_lib.to_wire(orc, m["u"])) == dv["bases"][1]           # G' = u o (G | H)
    assert int.from_bytes(w["proof"][48:80], "little") == m["r_p"]
    D = orc.g1_add_jac(c["B"], orc.g1_msm(dv["bases"][0], subarg_lib.to_wire(orc, m["d_scalars"])))  # the D task of the prover
    assert orc.g1_eq_jac(D, dv["stmt"][2])


def test_shim_says_where_the_reference_panics(orc):
    ell, nb = 3, 1
    c = gl.gp_inputs(21, ell, nb)
    d = gl.seeded_draws(orc, 22, ell, nb)
    assert gl.gp_prove(c, d)["ok"]
    b = subarg_lib.to_ints(orc, c["b"])
    b[0] = 0
    w = gl.gp_prove(dict(c, b=subarg_lib.to_wire(orc, b)), d)
    assert not w["ok"] and w["proof"] == bytes(gl.proof_bytes(2)) and w["state"] == c["state_in"] and w["challenges"] == bytes(gl.n_challenges(2) * FR)


# ---- gprod_algebra.hpp against integers ----
def test_scan_at_every_length_up_to_two_per_thread_and_one(emul, orc):
    """ell = 1 .. 2 T + 1: a chunk boundary at every position; below, at and above one and two elements per thread"""
    b = _ints(orc, 900, 2 * T + 1)
    for ell in range(1, 2 * T + 2):
        got = emul("scan", T, ell, *["%x" % v for v in b[:ell]])
        assert got["c"] == gl.model_products(b[:ell]) and got["differ"] == 0, ell


@pytest.mark.parametrize("ell", [5, T, 2 * T + 1])
def test_scan_with_a_zero_factor(emul, orc, ell):
    b = _ints(orc, 901, ell)
    for at in (0, ell // 2, ell - 1):
        z = list(b)
        z[at] = 0
        got = emul("scan", T, ell, *["%x" % v for v in z])["c"]
        assert got == gl.model_products(z) and got[:at + 1] == gl.model_products(b)[:at + 1] and got[at + 1:] == [0] * (ell - at - 1)


@pytest.mark.parametrize("workers", [1, 7, T])
def test_scan_does_not_depend_on_the_workers(emul, orc, workers):
    b = _ints(orc, 902, 300)
    got = emul("scan", workers, 300, *["%x" % v for v in b])
    assert got["c"] == gl.model_products(b) and got["differ"] == 0


@pytest.mark.parametrize("ell,nb", [(1, 0), (1, 1), (1, 3), (4, 4), (124, 4), (2 * T + 1, 3), (3, 2 * T + 1)])
def test_layer_matches_the_integer_model(emul, orc, ell, nb):
    """u, vec_d, D's scalars, r_p and inner_prod; (1, 0): one factor and no blinder"""
    v = _ints(orc, 910 + ell + nb, 3 + ell + 2 * nb)
    alpha, beta, result = v[:3]
    b, rb, cbl = v[3:3 + ell], v[3 + ell:3 + ell + nb], v[3 + ell + nb:]
    got = emul("layer", T, ell, nb, *["%x" % x for x in v])
    want = gl.model_layer(b, rb, cbl, result, alpha, beta)
    assert got["r_p"] == want["r_p"] and got["inner_prod"] == want["inner_prod"]
    assert got["u"] == want["u"] and got["d"] == want["d"] and got["dsc"] == want["d_scalars"]
    assert got["uv"] == want["u"]                                                     # the verifier's vec_u (grand_product_argument.rs:214-220)
    # what the layer is for: <c, d> = inner_prod when gprod_result is the product (grand_product_argument.rs:148)
    prod = 1
    for x in b:
        prod = prod * x % R_
    c = gl.model_products(b) + cbl
    w = gl.model_layer(b, rb, cbl, prod, alpha, beta)
    assert sum(x * y for x, y in zip(c, w["d"])) % R_ == w["inner_prod"]


# ---- gprod_plan.hpp against the model ----
@pytest.mark.parametrize("count,ell,nb", [(1, 1, 1), (3, 6, 2), (5, 8, 0), (2, 124, 4), (7, 1, 3)])
def test_plan_matches_the_model(emul, count, ell, nb):
    p = emul("plan", count, ell, nb)
    m = gl.PlanModel(count, ell, nb)
    assert p["status"] == 0 and p["n"] == m.n and p["L"] == m.L
    assert p["draws_each"] == m.draws_each and p["challenges"] == m.challenges and p["proof_bytes"] == m.proof_bytes and p["bytes"] == [0, 48, 80]
    assert p["sp"] == [m.fr_wit, m.fr_draws, m.fr_rd, m.fr_z, m.fr_ab]
    names = ("result", "b", "rb", "cbl", "u", "dsc", "rdu", "rp", "chal")
    assert p["fr"] == [m.fr[k][0] for k in names] + [m.fr_total]
    at = m.fr_ab + 2 * count                                                          # disjoint and in order, right behind the IPA prover's
    for k in names:
        assert m.fr[k][0] == at
        at += m.fr[k][1]
    assert at == m.fr_total
    assert p["pt"] == [m.pt_B0, m.jac_total, m.aff_total] and p["res"] == [0, count, 2 * count] and 2 * count <= max(m.L * count * 4, 2 * count)
    assert p["by"] == [m.by_B, m.by_C, m.by_total] and p["flags"] == [count, 2 * count]
    assert p["ix"] == [m.ix_addend, m.ix_total] and p["addend"] == m.addend
    assert p["task"] == [m.task_C, m.task_D, m.task_total]
    assert p["msm"] == [1, count, count * m.n, m.n]
    # the totals the engine reserves by: the end of the last region of every kind at this depth — C and D share the loop's result memory,
    # so the sums end at the larger of the two — with C and r_p and two challenges ahead of the inner-product proof's; the IPA prover's
    # own totals end where this layer's regions begin, and nothing leads there
    assert p["totals"] == [m.fr_total, m.jac_total, m.aff_total, m.by_total, p["flags"][1], m.ix_total, m.task_total, max(p["loop_results"], p["res"][2]), 80, 2]
    assert p["loop_results"] == m.L * count * 4
    core = p["totals_core"]
    assert core[:4] == [m.fr["result"][0], m.pt_B0, m.aff_total - count, m.by_B] and core[4:] == [count, m.ix_addend, m.task_C, p["loop_results"], 0, 0]
    # the proof bytes: C, r_p, then the inner-product proof of tests/subarg_verify_lib.py
    assert m.proof_bytes == 80 + sv.proof_bytes(IPA, m.L)


@pytest.mark.parametrize("count,ell,nb", [(1, 1, 0), (3, 6, 2), (2, 124, 4)])
def test_verifier_plan_lies_behind_the_inner_product_check(emul, count, ell, nb):
    """GprodCheckPlan: regions disjoint and in order behind SubargCheckPlan's (tests/subarg_verify_lib.py says its row and bytes)"""
    p = emul("check", count, ell, nb)
    n = ell + nb
    L = gl.log2(n)
    NP, PP, by, fr, ix, fr_z, fr_u = p["sp"]
    assert p["status"] == 0 and NP == n + 4 * L + 5 and PP == 2 + 4 * L and fr_u == fr_z + count
    assert p["proof"] == [80 + sv.proof_bytes(IPA, L), 48, 4 + L] and p["proof"][0] == gl.proof_bytes(L)
    h = (by + 15) // 16 * 16
    assert p["by"] == [h, h + 80 * count, h + 128 * count, h + 176 * count]
    assert p["st"] == [count * PP + count, count * PP + 2 * count, count * PP + 3 * count]
    assert p["fr"] == [fr, fr + count, fr + 2 * count, fr + 3 * count, fr + 5 * count]
    assert p["ix"] == [ix, ix + count, ix + 2 * count, ix + 3 * count]
    assert p["aff"] == [k * count for k in range(6)]
    stmt = n + PP                                                                     # the row: G | H, the inner proof's points, crs_U C D
    assert p["lists"] == [80 * i for i in range(count)] + [i * NP + stmt + 1 for i in range(count)] + [i * NP + stmt for i in range(count)]
    # the totals: the end of the last region of every kind (crs_U and B lie within the check's 3 count Jacobian inputs; one task and one
    # sum per item), the head of 80 bytes and two challenges ahead of the inner-product proof's; the check's own totals below them
    assert p["totals"] == [p["fr"][4], 3 * count, p["aff"][5], p["by"][3], p["st"][2], p["ix"][3], count, count, 80, 2]
    assert p["totals_core"] == [fr, 3 * count, 0, by, count * PP + count, ix, count, count, 0, 0]
    assert emul("check", 1, 3, 0)["status"] == 1 and emul("check", 65537, 3, 1)["status"] == 2


def test_plan_refuses_what_the_reference_cannot_run(emul):
    assert emul("plan", 1, 0, 4)["status"] == 3                                       # ell = 0
    assert emul("plan", 1, 1, 0)["status"] == 4                                       # n = 1
    for ell, nb in ((3, 0), (2, 1), (4, 2)):
        assert emul("plan", 1, ell, nb)["status"] == 1
    assert emul("plan", 16385, 3, 1)["status"] == 2 and emul("plan", 16384, 3, 1)["status"] == 0
    assert emul("plan", (1 << 24) // (2 * 4096 + 2) + 1, 4092, 4)["status"] == 2
    assert emul("plan", 0, 3, 1)["status"] == 0


# ---- the model of steps 1 and 2 ----
def test_python_model_of_steps_1_and_2_is_the_oracles(orc):
    """the model the GPU test searches entry states with: continued through beta and the inner-product prover's transcript it ends in
    the oracle's state"""
    ell, nb, L = 3, 1, 2
    for filler in (b"", bytes(41), bytes(165)):
        c = gl.gp_inputs(7200, ell, nb, filler=filler)
        w = gl.gp_prove(c, gl.seeded_draws(orc, 7201, ell, nb))
        dv = gl.gp_derive(c, gl.seeded_draws(orc, 7201, ell, nb)[:nb * FR])
        ipa = w["proof"][80:]
        t = gl.model_steps(orc, c, w["proof"][:48], int.from_bytes(w["proof"][48:80], "little"))
        chal = [subarg_lib.to_ints(orc, w["challenges"][:FR])[0], t.get_and_append_challenge(b"gprod_beta")[0]]
        assert subarg_lib.state_bytes(t.to_words()) == dv["state"]
        for enc in (w["proof"][:48], orc.g1_compress_jac(dv["stmt"][2])):
            t.append_message(b"ipa_step1", enc)
        t.append_scalar(b"ipa_step1", subarg_lib.to_ints(orc, dv["z"])[0])
        for k in range(2):
            t.append_message(b"ipa_step1", ipa[48 * k:48 * (k + 1)])
        chal += [t.get_and_append_challenge(b"ipa_alpha")[0], t.get_and_append_challenge(b"ipa_beta")[0]]
        for j in range(L):
            for name in sv.ROUND_ORDER[IPA]:
                t.append_message(b"ipa_loop", sv.point(ipa, sv.slot(IPA, L, name, j)))
            chal.append(t.get_and_append_challenge(b"ipa_gamma")[0])
        assert subarg_lib.state_bytes(t.to_words()) == w["state"] and subarg_lib.to_wire(orc, chal) == w["challenges"]


# ---- names ----
def test_names_agree_in_header_exports_and_library():
    from curdleproofs_amd.build import build
    build()
    import curdleproofs_amd as cpx
    lib = cpx.load_library()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "cpx.h")).read()
    for name in NAMES:
        assert name in cpx.EXPORTS
        assert hasattr(lib, name), "libcpx.so does not export %s" % name
        assert re.search(r"pub fn %s\(" % name, ffi), "integration/rust/ffi.rs lacks %s" % name
        assert re.search(r"\bint %s\(" % name, hdr), "include/cpx.h lacks %s" % name
    for cite in ("grand_product_argument.rs:43-166", "grand_product_argument.rs:180-246", ":248-253", ":86"):
        assert cite in hdr
    assert callable(cpx.Context.gprod_prove) and callable(cpx.Context.gprod_verify)
    for k in ("k_gprod_products", "k_gprod_setup", "k_gprod_rdu", "k_gprod_verify_steps"):
        assert k in cpx.Context.KERNELS
    assert "gprod.hip" in __import__("curdleproofs_amd.build", fromlist=["SOURCES"]).SOURCES
    assert gl.THREADS == int(re.search(r"GPROD_THREADS = (\d+)", open(os.path.join(ROOT, "curdleproofs_amd", "csrc", "kernels.h")).read()).group(1))
