"""CPU side of cpx_ipa_verify / cpx_same_msm_verify: the plan header compiled for the CPU (tests/host_emul/subarg_check_plan_emul.cpp,
plain and sanitized) against the layout restated in tests/subarg_verify_lib.py and a Python-integer model of the weights; the flattened
check itself against the oracle — for the oracle's valid proofs the planned row of points with the planned weights sums to the identity
(the oracle's group calls), and after every single change the GPU test makes it does not, while the oracle's own verifier rejects; the new
names in the header, EXPORTS and the library; the size formulas against the oracle's serialised lengths."""
import os
import re
import subprocess

import pytest

from tests import subarg_lib, subarg_verify_lib as sv
from tests.check_harness import build_emul
from tests.subarg_lib import IPA, SMSM, R_

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FR, AFF, JAC = 32, 96, 144
KINDS = pytest.mark.parametrize("kind", [IPA, SMSM], ids=["ipa", "same_msm"])
NAMES = ("cpx_ipa_verify", "cpx_same_msm_verify")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    exe = build_emul("subarg_check_plan_emul.cpp", ["subarg_check_plan.hpp", "tier0_plan.hpp", "mont32.hpp", "modinv30.hpp"], request.param == "sanitized", hip=False)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout       # a sanitizer report is a non-zero exit
        res = {"base_off": {}, "scalar_byte": {}, "block": {}, "round": {}}
        for line in out.splitlines():
            key, *vals = line.split()
            if key == "row":
                res["row"] = [int(v, 16) for v in vals]
                continue
            vals = [int(v) for v in vals]
            if key in ("base_off", "scalar_byte"):
                res[key][vals[0]] = vals[1]
            elif key in ("block", "round"):
                res[key][vals[0]] = vals[1:]
            else:
                res[key] = vals[0] if len(vals) == 1 and not key.startswith("idx_") else vals
        return res

    return run


def emul_row(emul, kind, n, a, chal, fin, z=0, u=()):
    args = list(a) + list(chal) + list(fin) + ([z] + list(u) if kind == IPA else [])
    return emul("row", kind, n, *["%x" % (v % R_) for v in args])["row"]


# ---- the layout ----
@pytest.mark.parametrize("count,n", [(1, 1), (1, 2), (3, 8), (2, 64)])
@KINDS
def test_plan_layout(emul, kind, count, n):
    L = sv.log2(n)
    p = emul("plan", kind, count, n)
    pp, pb, fam = sv.proof_points(kind, L), sv.proof_bytes(kind, L), sv.FAMILIES[kind]
    points = fam * n + pp + 3
    assert points == (n + 1 + 4 * L + 4 if kind == IPA else 3 * n + 6 * L + 6)                     # the issue's count of an item's points
    assert p["status"] == 0 and p["L"] == L and p["checks"] == sv.CHECKS[kind] and p["families"] == fam
    assert (p["proof_points"], p["proof_bytes"], p["challenges"], p["points"]) == (pp, pb, sv.n_challenges(kind, L), points)
    assert p["base_off"] == {f: f * n for f in range(fam)} and p["proof_off"] == fam * n and p["statement_off"] == fam * n + pp
    assert p["scalar_byte"] == {i: sv.scalar_at(kind, L, i) for i in range(2 if kind == IPA else 1)}
    for b, name in enumerate(sv.BLOCKS[kind]):                                                      # blocks in byte order
        right, check, first = p["block"][b]
        assert right == (name[0] == "R") and check == (("C", "D") if kind == IPA else ("A", "T", "U")).index(name[2])
        assert L == 0 or first == sv.slot(kind, L, name, 0)
    for j in range(L):                                                                              # a round's points in transcript order
        assert p["round"][j] == [sv.slot(kind, L, name, j) for name in sv.ROUND_ORDER[kind]]
    # memory: disjoint consecutive segments
    wts, z, u, rnd, ch, total = p["fr"]
    assert (wts, z) == (0, count * points) and u - z == (count if kind == IPA else 0) and rnd - u == (count * n if kind == IPA else 0)
    assert ch - rnd == count * sv.CHECKS[kind] and total - ch == count * sv.n_challenges(kind, L)
    prf, st, tu, btotal = p["by"]
    assert prf == 0 and count * pb <= st < count * pb + 16 and st % 16 == 0 and tu - st == count * 3 * 48
    assert btotal - tu == (0 if kind == IPA else count * 2 * n * 48)
    assert p["ix"] == [0, count * pp, 2 * count * pp, 2 * count * pp + 3 * count]
    # the decoder reads proof point s of item i where it lies and writes it into the item's row; the normaliser likewise
    assert p["idx_src"] == [i * pb + 48 * s for i in range(count) for s in range(pp)]
    assert p["idx_dst"] == [i * points + fam * n + s for i in range(count) for s in range(pp)]
    assert p["idx_statement"] == [i * points + fam * n + pp + k for i in range(count) for k in range(3)]
    assert p["msm"] == [1, count, count * points, points]                                           # one task per item, its row
    # status bytes: the decoder's verdicts, then the items' flags; Jacobian inputs: the statement points; no dense affine points
    assert p["st"] == [count * pp, count * pp + count] and p["jac"] == 3 * count and p["aff"] == 0
    # the totals the engine reserves by: the end of the last region of every kind (Fr, Jacobian, affine, bytes, status, index words; one
    # task and one sum per item), and nothing leads the proof or its challenges at this depth
    assert p["totals"] == [total, p["jac"], p["aff"], btotal, p["st"][1], p["ix"][3], count, count, 0, 0]


@KINDS
def test_limits(emul, kind):
    for n in (0, 3, 6, 12):
        assert emul("limit", kind, 1, n)["status"] == 1
    assert emul("limit", kind, 1 << 16, 1)["status"] == 0 and emul("limit", kind, (1 << 16) + 1, 1)["status"] == 2     # 2^16 tasks
    n, L = 1 << 12, 12
    per = n + 4 * L + 5 if kind == IPA else 3 * n + 6 * L + 6
    most = (1 << 24) // per
    assert emul("limit", kind, most, n)["status"] == 0 and emul("limit", kind, most + 1, n)["status"] == 2               # 2^24 points
    assert emul("limit", kind, 1, 1 << 25)["status"] == 2
    assert emul("limit", kind, 0, 8)["status"] == 0


# ---- the weights against integers ----
@pytest.mark.parametrize("n", [1, 2, 8, 64])
@KINDS
def test_rows_match_the_integer_model(emul, orc, kind, n):
    L = sv.log2(n)
    ints = subarg_lib.to_ints(orc, orc.rng(900 + 10 * n + kind).fr(sv.CHECKS[kind] + sv.n_challenges(kind, L) + 3 + n))
    it = iter(ints)
    a = [next(it) for _ in range(sv.CHECKS[kind])]
    chal = [next(it) for _ in range(sv.n_challenges(kind, L))]
    fin = [next(it) for _ in range(2 if kind == IPA else 1)]
    z, u = (next(it), [next(it) for _ in range(n)]) if kind == IPA else (0, ())
    got = emul_row(emul, kind, n, a, chal, fin, z, u)
    assert got == sv.model_row(kind, n, a, chal, fin, z, u)
    assert len(got) == sv.FAMILIES[kind] * n + sv.proof_points(kind, L) + 3


# ---- the flattened check against the oracle ----
def row_points(orc, c):
    """the item's row of points as the plan lays it out, affine"""
    kind, L = c["kind"], sv.log2(c["n"])
    enc = c["proof"][:48 * sv.proof_points(kind, L)]
    return b"".join(c["bases"]) + orc.g1_decompress(enc) + orc.g1_to_affine(b"".join(c["stmt"]))


def flattened_sum_is_identity(emul, orc, c, rand, o):
    kind, n = c["kind"], c["n"]
    L = sv.log2(n)
    a, chal = subarg_lib.to_ints(orc, rand), subarg_lib.to_ints(orc, o["challenges"])
    fin = [sv.scalar(kind, L, c["proof"], i) for i in range(2 if kind == IPA else 1)]
    z, u = (subarg_lib.to_ints(orc, c["z"])[0], subarg_lib.to_ints(orc, c["vec_u"])) if kind == IPA else (0, ())
    row = emul_row(emul, kind, n, a, chal, fin, z, u)
    total = orc.g1_msm(row_points(orc, c), subarg_lib.to_wire(orc, row))
    return total[2 * 48:] == bytes(48)                                                              # Z = 0


@pytest.mark.parametrize("n", [1, 2, 8])
@KINDS
def test_flattened_check_is_the_accumulators_verdict(emul, orc, kind, n):
    c = sv.make(kind, 7000 + 10 * n + kind, n, filler=bytes(n))
    rand = sv.factors(orc, 11 * n + kind, kind)
    o = sv.verify(c, rand)
    assert o["verdict"] == sv.OK and o["state"] != c["state_in"]
    assert flattened_sum_is_identity(emul, orc, c, rand, o)
    muts = sv.mutations(orc, c)
    assert len(muts) >= (3 if n == 1 else 4)
    for name, m in muts.items():
        om = sv.verify(m, rand)
        assert om["verdict"] == sv.ERR_VERIFY, name
        assert not flattened_sum_is_identity(emul, orc, m, rand, om), name


@pytest.mark.parametrize("n", [1, 2, 8])
@KINDS
def test_python_transcript_model_is_the_oracles(orc, kind, n):
    """the model the GPU test searches entry states with (which filler puts a point, a label, a header across the rate boundary)"""
    for filler in (b"", bytes(41), bytes(165)):
        c = sv.make(kind, 7200 + 10 * n + kind, n, filler=filler)
        o = sv.verify(c, sv.factors(orc, 3, kind))
        t, chal = sv.model_transcript(orc, c)
        assert subarg_lib.state_bytes(t.to_words()) == o["state"] and subarg_lib.to_wire(orc, chal) == o["challenges"]


@KINDS
def test_undecodable_bytes_never_reach_verify(orc, kind):
    c = sv.make(kind, 7100 + kind, 4)
    rand = sv.factors(orc, 5 + kind, kind)
    bad = dict(c, proof=sv.with_scalar(kind, 2, c["proof"], 0, R_))                                 # a scalar equal to r
    o = sv.verify(bad, rand)
    assert o["verdict"] == sv.ERR_DESERIALIZE and o["state"] == c["state_in"] and o["challenges"] == bytes(len(o["challenges"]))


# ---- names and sizes ----
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
    for cite in ("inner_product_argument.rs:202-326", "same_multiscalar_argument.rs:153-261", "inner_product_argument.rs:328-338",
                 "same_multiscalar_argument.rs:263-275", "msm_accumulator.rs:37-68"):
        assert cite in hdr
    assert callable(cpx.Context.ipa_verify) and callable(cpx.Context.same_msm_verify)
    assert "k_subarg_scalars" in cpx.Context.KERNELS
    assert "subarg.hip" in __import__("curdleproofs_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.mark.parametrize("L", [0, 1, 3, 8])
def test_size_formulas_are_the_oracles_serialised_lengths(L):
    assert sv.serialized_len(IPA, L) == 48 * (2 + 4 * L) + 64 == sv.proof_bytes(IPA, L)
    assert sv.serialized_len(SMSM, L) == 48 * (3 + 6 * L) + 32 == sv.proof_bytes(SMSM, L)
