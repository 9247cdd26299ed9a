"""CPU side of cpx_ipa_prove / cpx_same_msm_prove: the new oracle shim (tests/subarg_prove_lib.py) pinned to the one the loop tests have
used (tests/subarg_lib.py `case`); the blinder header compiled for the CPU (tests/host_emul/subarg_prove_plan_emul.cpp, plain and
sanitized) against generate_ipa_blinders on Python integers; the plan header against a Python model of the layout and against the proof
byte order of tests/subarg_verify_lib.py; the model of step 1 the GPU test searches entry states with against the oracle; the new names
in the header, EXPORTS, the Rust source and the library."""
import os
import re
import subprocess

import pytest

from tests import subarg_lib, subarg_prove_lib as sp, subarg_verify_lib as sv
from tests.check_harness import build_emul
from tests.subarg_lib import IPA, SMSM, R_

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FR, AFF, JAC = 32, 96, 144
KINDS = pytest.mark.parametrize("kind", [IPA, SMSM], ids=["ipa", "same_msm"])
NAMES = ("cpx_ipa_prove", "cpx_same_msm_prove", "cpx_ipa_prove_rng", "cpx_same_msm_prove_rng")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    deps = ["subarg_prove_plan.hpp", "blinder_algebra.hpp", "loop_plan.hpp", "tier0_plan.hpp", "mont32.hpp", "modinv30.hpp"]
    exe = build_emul("subarg_prove_plan_emul.cpp", deps, request.param == "sanitized", hip=False)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout       # a sanitizer report is a non-zero exit
        res = {"first_family": {}, "scalar_byte": {}, "block": {}}
        for line in out.splitlines():
            key, *vals = line.split()
            if key == "rd":
                res["rd"] = [int(v, 16) for v in vals]
                continue
            vals = [int(v) for v in vals]
            if key in ("first_family", "scalar_byte"):
                res[key][vals[0]] = vals[1]
            elif key == "block":
                res[key][vals[0]] = (vals[1], vals[2:])
            else:
                res[key] = vals[0] if len(vals) == 1 else vals
        return res

    return run


# ---- the new shim is the old one ----
@pytest.mark.parametrize("n,pad", [(2, 0), (8, 0), (8, 3), (16, 4)])
@KINDS
def test_new_shim_gives_what_the_old_one_exports(orc, kind, n, pad):
    """sub_ipa / sub_samemsm run the oracle's provers on inputs they keep to themselves; sp_inputs draws the same inputs from the same
    seed and sp_prove, fed with them and the same draws, returns the same proof bytes and end state"""
    for seed, filler in ((7000 + 10 * n + kind, b""), (7001 + 10 * n + kind, bytes(41))):
        old = subarg_lib.case(kind, seed, n, pad=pad, filler=filler)
        c = sp.sp_inputs(kind, seed, n, pad=pad, filler=filler)
        assert c["bases"][0] == old["bases"][0] and c["bases"][1] == old["bases"][1] and c["state_in"] == subarg_lib.entry_state(filler)
        if kind == SMSM:
            assert c["bases"][2] == old["bases"][2]
        w = sp.sp_prove(c, sp.seeded_draws(orc, kind, seed, n))
        assert w["ok"] and w["proof"] == old["proof"] and w["state"] == old["state_out"]
        L = sv.log2(n)
        assert w["proof"][:48 * sv.FIRST[kind]] == old["pre"]
        gam = w["challenges"][FR * (2 if kind == IPA else 1):]
        assert gam == subarg_lib.model_loop(orc, kind, n, old["bases"], old["vecs"], old["state_in"])["gammas"] and len(gam) == L * FR


@KINDS
def test_consistent_statements_are_consistent(orc, kind):
    n = 4
    c = sp.sp_inputs(kind, 31, n, consistent=True, pad=1)
    ints = lambda w: subarg_lib.to_ints(orc, w)
    if kind == IPA:
        G, Gp = c["bases"]
        assert orc.g1_scale(G, c["vec_u"]) == Gp and Gp[AFF * (n - 1):] == bytes(AFF)
        assert orc.g1_eq_jac(orc.g1_msm(G, c["vecs"][0]), c["stmt"][1]) and orc.g1_eq_jac(orc.g1_msm(Gp, c["vecs"][1]), c["stmt"][2])
        assert sum(a * b for a, b in zip(ints(c["vecs"][0]), ints(c["vecs"][1]))) % R_ == ints(c["z"])[0]
    else:
        for f in range(3):
            assert orc.g1_eq_jac(orc.g1_msm(c["bases"][f], c["vecs"][0]), c["stmt"][f])
    w = sp.sp_prove(c, sp.seeded_draws(orc, kind, 31, n))
    vc = dict(c, bases=c["bases"][:1] if kind == IPA else c["bases"], proof=w["proof"])
    o = sv.verify(vc, sv.factors(orc, 5, kind))
    assert o["verdict"] == sv.OK and o["state"] == w["state"] and o["challenges"] == w["challenges"]


# ---- the blinder header against integers ----
def emul_blinders(emul, c, d, r, z, workers):
    return emul("blinders", len(c), workers, *["%x" % (v % R_) for v in list(c) + list(d) + list(r) + list(z)])


def _ints(orc, seed, k):
    return subarg_lib.to_ints(orc, orc.rng(seed).fr(k))


@pytest.mark.parametrize("n,workers", [(2, 128), (4, 1), (8, 128), (64, 128), (256, 128), (256, 7)])
def test_blinders_match_the_integer_model(emul, orc, n, workers):
    """n = 2: no free z, delta an empty sum; n = 256: more elements than a work-group has threads"""
    v = _ints(orc, 900 + n, 4 * n - 2)
    c, d, r, z = v[:n], v[n:2 * n], v[2 * n:3 * n], v[3 * n:]
    got = emul_blinders(emul, c, d, r, z, workers)
    want = sp.model_blinders(c, d, r, z)
    assert got["singular"] == 0 and got["rd"] == want
    dot = lambda a, b: sum(x * y for x, y in zip(a, b)) % R_
    assert (dot(r, d) + dot(want, c)) % R_ == 0 and dot(r, want) == 0       # <r, d> + <z, c> = 0 and <r, z> = 0


@pytest.mark.parametrize("n", [2, 8])
def test_the_two_singular_cases_are_flagged(emul, orc, n):
    v = _ints(orc, 950 + n, 4 * n - 2)
    c, d, r, z = v[:n], v[n:2 * n], v[2 * n:3 * n], v[3 * n:]
    c0 = list(c)
    c0[n - 2] = 0                                                            # inner_product_argument.rs:69
    assert sp.model_blinders(c0, d, r, z) is None and emul_blinders(emul, c0, d, r, z, 128)["singular"] == 1
    r0 = list(r)
    r0[n - 1] = r[n - 2] * c[n - 1] * pow(c[n - 2], R_ - 2, R_) % R_         # :71: the denominator is zero
    assert sp.model_blinders(c, d, r0, z) is None and emul_blinders(emul, c, d, r0, z, 128)["singular"] == 1
    assert emul_blinders(emul, c, d, r, z, 128)["singular"] == 0


def test_the_oracle_shim_refuses_the_same_two_cases(orc):
    n = 4
    base = sp.sp_inputs(IPA, 77, n, filler=b"x")
    draws = sp.seeded_draws(orc, IPA, 77, n)
    c, r = subarg_lib.to_ints(orc, base["vecs"][0]), subarg_lib.to_ints(orc, draws)
    c0 = list(c)
    c0[n - 2] = 0
    r0 = list(r)
    r0[n - 1] = r[n - 2] * c[n - 1] * pow(c[n - 2], R_ - 2, R_) % R_
    for it, dr in ((dict(base, vecs=(subarg_lib.to_wire(orc, c0), base["vecs"][1])), draws), (base, subarg_lib.to_wire(orc, r0))):
        w = sp.sp_prove(it, dr)
        assert not w["ok"] and w["state"] == base["state_in"] and w["proof"] == bytes(len(w["proof"])) and w["challenges"] == bytes(len(w["challenges"]))
    assert sp.sp_prove(base, draws)["ok"]


# ---- the layout ----
def model_loop_plan(kind, count, n):
    """loop_plan.hpp's totals (tests/test_loop_rounds_cpu.py checks that header): (Fr words, results, tasks of all rounds)"""
    L = sv.log2(n)
    terms = 4 if kind == IPA else 6
    vec, row = ((4, 2 * n + 2) if kind == IPA else (2, n))
    fr = count * vec * n + count * row + (count if kind == IPA else 0) + count * L + count * (2 if kind == IPA else 1)
    return fr, L * count * terms, L * count * terms


@pytest.mark.parametrize("count,n", [(1, 1), (1, 2), (3, 8), (2, 64), (5, 256)])
@KINDS
def test_plan_layout(emul, kind, count, n):
    p = emul("plan", kind, count, n)
    L = sv.log2(n)
    first, nvec, de, ab = sv.FIRST[kind], sp.NVEC[kind], sp.draws_each(kind, n), (2 if kind == IPA else 1)
    if kind == IPA and n == 1:
        de = 0                                                               # (the engine refuses the IPA at n = 1 before the plan is used)
        assert p["draws_each"] == 0
    loop_fr, results, loop_tasks = model_loop_plan(kind, count, n)
    assert p["status"] == 0 and p["loop"] == [loop_fr, results, loop_tasks]
    assert (p["L"], p["first"], p["nvec"], p["draws_each"], p["ab_each"], p["challenges"]) == (L, first, nvec, de, ab, sv.n_challenges(kind, L))
    assert (p["blocks"], p["proof_points"], p["proof_bytes"], p["points"]) == (len(sv.BLOCKS[kind]), sv.proof_points(kind, L), sv.proof_bytes(kind, L), count * (first + 3))
    # memory: disjoint consecutive segments behind the loop's
    wit, draws, rd, z, abo, total = p["fr"]
    assert wit == loop_fr and draws - wit == count * nvec * n and rd - draws == count * de and z - rd == (count * n if kind == IPA else 0)
    assert abo - z == (count if kind == IPA else 0) and total - abo == count * ab
    pts, tu, rng, btotal = p["by"]
    assert pts == results * 48 and tu - pts == count * (first + 3) * 48 and rng - tu == (0 if kind == IPA else count * 2 * n * 48) and btotal - rng == count * 40
    assert rng % 16 == 0                                                     # the rng states are read as words
    assert p["aff"] == [results, results + count * (first + 3)] and p["task"] == [loop_tasks, loop_tasks + count * first]
    assert p["pt"] == [0, count * first - 1, count * first, count * (first + 3) - 1]
    assert p["first_family"] == {b: b for b in range(first)}
    assert p["msm"] == [1, count * first, count * first * n, n]              # the B points: item-major tasks of n points
    # the totals the engine reserves by: the end of the last region of every kind (Fr, Jacobian, affine, bytes, flags: one per item, index
    # words: the loop's lists, tasks, sums: the loop's results), and nothing leads the proof or its challenges at this depth
    idx = 2 * L * (n // 2 + (1 if kind == IPA else 0))
    assert p["totals"] == [total, count * (first + 3), p["aff"][1], btotal, count, idx, p["task"][1], results, 0, 0]


@pytest.mark.parametrize("n", [1, 2, 8])
@KINDS
def test_proof_bytes_are_laid_out_as_serialize_writes_them(emul, kind, n):
    """the host puts the proof together from sp.round_slot / block_term / scalar_byte: against tests/subarg_verify_lib.py `slot`"""
    L = sv.log2(n)
    p = emul("plan", kind, 1, n)
    assert p["scalar_byte"] == {i: sv.scalar_at(kind, L, i) for i in range(2 if kind == IPA else 1)}
    for b, name in enumerate(sv.BLOCKS[kind]):
        term, slots = p["block"][b]
        assert sv.ROUND_ORDER[kind][term] == name                            # the cross term of a round this block collects
        assert slots == [sv.slot(kind, L, name, j) for j in range(L)]


@KINDS
def test_limits_are_the_loops(emul, kind):
    for n in (0, 3, 6, 12):
        assert emul("limit", kind, 1, n)["status"] == 1
    most = 16384 if kind == IPA else 10922
    assert emul("limit", kind, most, 2)["status"] == 0 and emul("limit", kind, most + 1, 2)["status"] == 2
    n = 1 << 12
    per = 2 * n + 2 if kind == IPA else 3 * n
    most = (1 << 24) // per
    assert emul("limit", kind, most, n)["status"] == 0 and emul("limit", kind, most + 1, n)["status"] == 2
    assert emul("limit", kind, 0, 8)["status"] == 0


# ---- the model of step 1 ----
@pytest.mark.parametrize("n", [2, 8])
@KINDS
def test_python_model_of_step_1_is_the_oracles(orc, kind, n):
    """the model the GPU test searches entry states with: continued through the challenges and the rounds it ends in the oracle's state"""
    from tests import strobe_ref
    for filler in (b"", bytes(41), bytes(165)):
        c = sp.sp_inputs(kind, 7200 + 10 * n + kind, n, filler=filler)
        w = sp.sp_prove(c, sp.seeded_draws(orc, kind, 7200, n))
        L = sv.log2(n)
        t = sp.model_step1(orc, c, w["proof"][:48 * sv.FIRST[kind]])
        chal = [t.get_and_append_challenge(b"ipa_alpha" if kind == IPA else b"same_msm_alpha")[0]]
        if kind == IPA:
            chal.append(t.get_and_append_challenge(b"ipa_beta")[0])
        for j in range(L):
            for name in sv.ROUND_ORDER[kind]:
                t.append_message(subarg_lib.LABELS[kind][0], sv.point(w["proof"], sv.slot(kind, L, name, j)))
            chal.append(t.get_and_append_challenge(subarg_lib.LABELS[kind][1])[0])
        assert subarg_lib.state_bytes(t.to_words()) == w["state"] and subarg_lib.to_wire(orc, chal) == w["challenges"]
        assert strobe_ref.RATE == 166


# ---- names ----
def test_names_agree_in_header_exports_and_library():
    from curdleproofs_amd.build import build
    build()
    import curdleproofs_amd as cpx
    lib = cpx.load_library()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "cpx.h")).read()
    rust = open(os.path.join(ROOT, "integration", "rust", "subargs_mi355x.rs")).read()
    for name in NAMES:
        assert name in cpx.EXPORTS
        assert hasattr(lib, name), "libcpx.so does not export %s" % name
        assert re.search(r"pub fn %s\(" % name, ffi), "integration/rust/ffi.rs lacks %s" % name
        assert re.search(r"\bint %s\(" % name, hdr), "include/cpx.h lacks %s" % name
    assert "cpx_ipa_prove(" in rust and "cpx_same_msm_prove(" in rust
    for cite in ("inner_product_argument.rs:98-199", "same_multiscalar_argument.rs:69-150", "inner_product_argument.rs:42-82"):
        assert cite in hdr or cite in open(os.path.join(ROOT, "curdleproofs_amd", "csrc", "blinder_algebra.hpp")).read()
    assert callable(cpx.Context.ipa_prove) and callable(cpx.Context.same_msm_prove)
    assert "k_subarg_blinders" in cpx.Context.KERNELS and "k_subarg_prove_setup" in cpx.Context.KERNELS
    assert "subarg_prove.hip" in __import__("curdleproofs_amd.build", fromlist=["SOURCES"]).SOURCES
