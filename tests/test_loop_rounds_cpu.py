"""CPU checks of the log-round loops as one call (cpx_ipa_rounds, cpx_same_msm_rounds) and of the transcript as a value
(cpx_transcript_*):
  * the five transcript calls against merlin's published vector, tests/strobe_ref.py and the oracle's Merlin (tests/subarg_lib.py);
  * curdleproofs_amd/csrc/loop_plan.hpp, compiled with g++ into tests/host_emul/loop_plan_emul.cpp (plain and with
    -fsanitize=address,undefined), against a model over the additive group Z_r: a "point" is an integer, an MSM a dot product;
  * the reference model of the loop that the GPU tests use (subarg_lib.model_loop) against the oracle's own ipa_new / samemsm_new;
  * the boundary: header, export list, library, Rust declarations."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from tests import strobe_ref, subarg_lib
from tests.check_harness import build_emul
from tests.subarg_lib import IPA, SMSM, R_

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("cpx_transcript_new", "cpx_transcript_append_message", "cpx_transcript_append_scalar", "cpx_transcript_challenge_bytes",
         "cpx_transcript_challenge_scalar", "cpx_ipa_rounds", "cpx_same_msm_rounds")
RATE = strobe_ref.RATE


@pytest.fixture(scope="module")
def lib():
    from curdleproofs_amd.build import build
    build()
    import curdleproofs_amd as cpx
    return cpx.load_library()


@pytest.fixture(scope="module")
def T(lib):
    from curdleproofs_amd.transcript import Transcript
    return Transcript


def mont(x):
    return strobe_ref.to_mont(x).to_bytes(32, "little")


# ---- the boundary ----
def test_names_are_exported_everywhere(lib):
    import curdleproofs_amd as cpx
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "cpx.h")).read()
    for name in NAMES:
        assert name in cpx.EXPORTS
        assert hasattr(lib, name), "libcpx.so does not export %s" % name
        assert re.search(r"pub fn %s\(" % name, ffi), "integration/rust/ffi.rs lacks %s" % name
        assert re.search(r"\bint %s\(" % name, hdr), "include/cpx.h lacks %s" % name
    assert "#define CPX_TRANSCRIPT_BYTES 216" in hdr and cpx.TRANSCRIPT_BYTES == 216
    for cite in ("inner_product_argument.rs:150-186", "same_multiscalar_argument.rs:99-136", "transcript.rs:41-54", "transcript.rs:29-33"):
        assert cite in hdr
    assert callable(cpx.Context.ipa_rounds) and callable(cpx.Context.same_msm_rounds)
    assert "loop.hip" in __import__("curdleproofs_amd.build", fromlist=["SOURCES"]).SOURCES


def test_loop_calls_refuse_null_without_a_device(lib):
    import curdleproofs_amd as cpx
    b = (ctypes.c_uint8 * 512)(*([0xaa] * 512))
    full = [b] * 10
    for hole in (0, 1, 2, 3, 4, 5, 8):                      # G, G', H, c, d, transcripts, finals: needed; the three others may be NULL
        args = list(full)
        args[hole] = None
        assert lib.cpx_ipa_rounds(None, 1, 2, *args) == cpx.CPX_ERR_ARG
    for hole in (0, 1, 2, 3, 4, 7):
        args = list(full[:9])
        args[hole] = None
        assert lib.cpx_same_msm_rounds(None, 1, 2, *args) == cpx.CPX_ERR_ARG
    assert lib.cpx_ipa_rounds(None, 1, 2, *full) == cpx.CPX_ERR_ARG          # no context
    assert bytes(b) == b"\xaa" * 512


# ---- the transcript as a value ----
def test_merlin_published_vector(T, orc):
    t = T.new(b"test protocol")
    t.append_message(b"some label", b"some data")
    out = t.challenge_bytes(b"challenge", 32)
    assert out.hex().startswith("d5a21972") and out.hex().endswith("0615")
    assert out == orc.merlin_test_vector()


def _pair(T, label):
    return T.new(label), strobe_ref.Transcript(label)


def _same(t, ref):
    assert subarg_lib.words(t.state) == ref.to_words()


def test_messages_that_end_on_before_and_after_the_rate_boundary(T):
    probe = strobe_ref.Transcript(b"curdleproofs")
    probe.append_message(b"m", b"")
    at = probe.to_words()[25]                                # where the data of a message under this label starts
    seen = []
    for n in (RATE - at - 1, RATE - at, RATE - at + 1, 2 * RATE - at, 0, 1, 500):
        t, ref = _pair(T, b"curdleproofs")
        msg = bytes((7 * i + n) & 0xff for i in range(n))
        t.append_message(b"m", msg)
        ref.append_message(b"m", msg)
        _same(t, ref)
        t.append_message(b"again", b"x")                     # ... and the state goes on correctly from there
        ref.append_message(b"again", b"x")
        _same(t, ref)
        seen += strobe_ref.ends(ref.trace)[1:2] if n else []      # (entry 0: the constructor's dom-sep message)
    assert seen[:4] == [RATE - 1, RATE, 1, RATE]             # one before the boundary, on it, one after, on it again a block later


def test_challenge_bytes_and_scalars_follow_the_reference(T):
    t, ref = _pair(T, b"curdleproofs")
    for n in (0, 1, 32, 64, RATE - 1, RATE, RATE + 1, 400):
        assert t.challenge_bytes(b"c", n) == ref.challenge_bytes(b"c", n)
        _same(t, ref)
    x = 0x1234567890abcdef << 100
    t.append_scalar(b"s", mont(x))
    ref.append_scalar(b"s", x)
    _same(t, ref)
    for _ in range(5):
        want, _tries = ref.get_and_append_challenge(b"ch")
        assert t.challenge_scalar(b"ch") == mont(want)
        _same(t, ref)


def test_a_challenge_that_retries(T):
    """about 9.4 % of the draws are refused (2^255 / r = 1.104): the first seed whose draw the reference model retries"""
    for seed in range(200):
        ref = strobe_ref.Transcript(b"retry")
        ref.append_message(b"seed", seed.to_bytes(4, "little"))
        want, tries = ref.get_and_append_challenge(b"ch")
        if tries > 1:
            break
    assert tries > 1 and ("attempt", False) in ref.trace
    t = T.new(b"retry")
    t.append_message(b"seed", seed.to_bytes(4, "little"))
    assert t.challenge_scalar(b"ch") == mont(want)
    _same(t, ref)


@pytest.mark.parametrize("filler", [b"", b"x", bytes(range(200))])
def test_state_round_trip_through_the_oracles_merlin(T, filler):
    """the oracle's Strobe128 exported as 27 words is the state the library computes, and either continues the other"""
    t = T.new(b"subarg")
    if filler:
        t.append_message(b"filler", filler)
    assert t.state == subarg_lib.entry_state(filler)
    u = T.from_state(subarg_lib.entry_state(filler))
    ref = strobe_ref.Transcript.from_words(subarg_lib.words(subarg_lib.entry_state(filler)))
    u.append_message(b"next", b"message")
    ref.append_message(b"next", b"message")
    _same(u, ref)


def test_malformed_states_are_refused_and_left_alone(lib, T):
    import curdleproofs_amd as cpx
    good = T.new(b"x").state
    out = (ctypes.c_uint8 * 64)(*([0xaa] * 64))
    for word, value in ((25, RATE), (25, 1 << 32), (25, (1 << 64) - 1), (26, RATE + 1), (26, 1 << 40)):
        w = subarg_lib.words(good)
        w[word] = value
        bad = subarg_lib.state_bytes(w)
        st = (ctypes.c_uint8 * 216).from_buffer_copy(bad)
        assert lib.cpx_transcript_append_message(st, b"l", 1, b"m", 1) == cpx.CPX_ERR_ARG
        assert lib.cpx_transcript_append_scalar(st, b"l", 1, mont(5)) == cpx.CPX_ERR_ARG
        assert lib.cpx_transcript_challenge_bytes(st, b"l", 1, out, 64) == cpx.CPX_ERR_ARG
        assert lib.cpx_transcript_challenge_scalar(st, b"l", 1, out) == cpx.CPX_ERR_ARG
        assert bytes(st) == bad and bytes(out) == b"\xaa" * 64
    for word, value in ((25, RATE - 1), (26, RATE)):         # the largest values a transcript writes
        w = subarg_lib.words(good)
        w[word] = value
        st = (ctypes.c_uint8 * 216).from_buffer_copy(subarg_lib.state_bytes(w))
        assert lib.cpx_transcript_append_message(st, b"l", 1, b"m", 1) == cpx.CPX_OK
    st = (ctypes.c_uint8 * 216).from_buffer_copy(good)
    assert lib.cpx_transcript_append_scalar(st, b"l", 1, R_.to_bytes(32, "little")) == cpx.CPX_ERR_ARG      # a scalar >= r
    assert lib.cpx_transcript_append_scalar(st, b"l", 1, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_transcript_append_message(st, None, 1, b"m", 1) == cpx.CPX_ERR_ARG
    assert lib.cpx_transcript_append_message(st, b"l", 1, None, 1) == cpx.CPX_ERR_ARG
    assert lib.cpx_transcript_append_message(None, b"l", 1, b"m", 1) == cpx.CPX_ERR_ARG
    assert lib.cpx_transcript_new(b"l", 1, None) == cpx.CPX_ERR_ARG
    assert bytes(st) == good


# ---- loop_plan.hpp on the CPU ----
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    exe = build_emul("loop_plan_emul.cpp", ["loop_plan.hpp", "tier0_plan.hpp"], request.param == "sanitized", hip=False)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout       # a sanitizer report is a non-zero exit
        res = {"term": [], "family": {}, "vec": {}, "list": {}}
        for line in out.splitlines():
            key, *vals = line.split()
            vals = [int(v) for v in vals]
            if key == "term":
                res["term"].append(dict(zip(("q", "family", "family_off", "hi", "has_h", "len", "vec", "right", "scal_off"), vals)))
            elif key in ("family", "vec"):
                res[key][vals[0]] = vals[1]
            elif key == "list":
                res["list"][(vals[0], vals[1])] = vals[2:]
            else:
                res[key] = vals if len(vals) > 1 else vals[0]
        return res
    return run


def _reference_loop(kind, n, fams, H, vecs, gammas):
    """the loops as the reference writes them, bases folded, over Z_r"""
    fams, vecs, out = [list(f) for f in fams], [list(v) for v in vecs], []
    dot = lambda a, b: sum(x * y for x, y in zip(a, b)) % R_
    m, j = n, 0
    while m > 1:
        m //= 2
        g = gammas[j]
        gi = pow(g, R_ - 2, R_)
        if kind == IPA:
            (G, Gp), (c, d) = fams, vecs
            out.append([(dot(G[m:2 * m], c[:m]) + H * dot(c[:m], d[m:2 * m])) % R_, dot(Gp[:m], d[m:2 * m]),
                        (dot(G[:m], c[m:2 * m]) + H * dot(c[m:2 * m], d[:m])) % R_, dot(Gp[m:2 * m], d[:m])])
            vecs = [[(c[i] + gi * c[m + i]) % R_ for i in range(m)], [(d[i] + g * d[m + i]) % R_ for i in range(m)]]
            fams = [[(G[i] + g * G[m + i]) % R_ for i in range(m)], [(Gp[i] + gi * Gp[m + i]) % R_ for i in range(m)]]
        else:
            x = vecs[0]
            out.append([dot(f[m:2 * m], x[:m]) for f in fams] + [dot(f[:m], x[m:2 * m]) for f in fams])
            vecs = [[(x[i] + gi * x[m + i]) % R_ for i in range(m)]]
            fams = [[(f[i] + g * f[m + i]) % R_ for i in range(m)] for f in fams]
        j += 1
    return out, [v[0] for v in vecs]


@pytest.mark.parametrize("n", [2, 4, 8, 32])
@pytest.mark.parametrize("kind", [IPA, SMSM], ids=["ipa", "same_msm"])
def test_all_msm_rounds_from_the_plan_equal_the_fold_based_loop(emul, kind, n):
    pl = emul("plan", kind, 3, n)
    L, terms, hn = n.bit_length() - 1, (4 if kind == IPA else 6), n // 2
    nfam, nvec = (2, 2) if kind == IPA else (3, 1)
    assert pl["status"] == 0 and pl["L"] == L and pl["terms"] == terms and pl["tasks"] == 3 * terms
    assert pl["base_stride"] == (2 * n + 1 if kind == IPA else 3 * n) and pl["vec_words"] == (4 if kind == IPA else 2) * n
    assert pl["row_words"] == (2 * n + 2 if kind == IPA else n) and pl["results"] == L * 3 * terms
    assert pl["round_points"] == 3 * sum(t["len"] for t in pl["term"]) and pl["msm"] == [1, 3 * terms, pl["round_points"], hn + (kind == IPA)]
    fr = pl["fr"]
    assert fr == sorted(fr) and fr[0] == 0 and fr[1] == 3 * pl["vec_words"] and fr[2] - fr[1] == 3 * pl["row_words"]
    assert fr[3] - fr[2] == (3 if kind == IPA else 0) and fr[4] - fr[3] == 3 * L and fr[5] - fr[4] == 3 * pl["finals_each"]
    rng = random.Random(1000 * n + kind)
    rnd = lambda k: [rng.randrange(R_) for _ in range(k)]
    fams, vecs, H, gammas = [rnd(n) for _ in range(nfam)], [rnd(n) for _ in range(nvec)], rng.randrange(R_), [rng.randrange(1, R_) for _ in range(L)]
    want_rounds, want_finals = _reference_loop(kind, n, fams, H, vecs, gammas)
    # the all-MSM form: one flat array of the item's ORIGINAL bases, a fold coefficient per base, the vectors folded in place
    flat = sum(fams, []) + ([H] if kind == IPA else [])
    assert len(flat) == pl["base_stride"] and (kind != IPA or flat[pl["h_index"]] == H)
    coef = [[1] * n for _ in range(nfam)]
    v = [list(w) for w in vecs]
    for j in range(L):
        half = n >> (j + 1)
        lo, hi = pl["list"][(j, 0)], pl["list"][(j, 1)]
        assert len(lo) == len(hi) == pl["idx_len"] == hn + (kind == IPA)
        assert sorted(lo[:hn] + hi[:hn]) == list(range(n))                     # every original index in exactly one of the two lists
        assert all(k & half == 0 for k in lo[:hn]) and all(k & half for k in hi[:hn])
        row = [None] * pl["row_words"]
        got = []
        for t in pl["term"]:
            idx = (hi if t["hi"] else lo)[:t["len"]]
            vec = v[t["vec"]]
            sc = [vec[(half if t["right"] else 0) + (k & (half - 1))] * coef[t["family"]][k] % R_ for k in idx[:hn]]
            if t["has_h"]:
                other = v[1 - t["vec"]]
                a, b = (vec[half:2 * half], other[:half]) if t["right"] else (vec[:half], other[half:2 * half])
                sc.append(sum(p * q for p, q in zip(a, b)) % R_)
                assert idx[hn] == pl["h_index"]
            for i, s in enumerate(sc):                                        # IPA: the tasks' scalars do not overlap; SameMSM: G, T and U fold alike
                assert row[t["scal_off"] + i] is None if kind == IPA else row[t["scal_off"] + i] in (None, s)      # and share one scalar vector
                row[t["scal_off"] + i] = s
            got.append(sum(flat[t["family_off"] + k] * s for k, s in zip(idx, sc)) % R_)
        assert None not in row and got == want_rounds[j]
        g = gammas[j]
        gi = pow(g, R_ - 2, R_)
        for f in range(nfam):
            for k in hi[:hn]:
                coef[f][k] = coef[f][k] * (g if pl["family"][f] == 1 else gi) % R_
        for w in range(nvec):
            p = g if pl["vec"][w] == 1 else gi
            v[w][:half] = [(v[w][i] + p * v[w][half + i]) % R_ for i in range(half)]
    assert [w[0] for w in v] == want_finals


def test_no_round_at_n_1(emul):
    for kind in (IPA, SMSM):
        pl = emul("plan", kind, 5, 1)
        assert pl["status"] == 0 and pl["L"] == 0 and pl["results"] == 0 and pl["idx_total"] == 0 and pl["list"] == {}


def test_limits_refuse_one_past_each_bound(emul):
    ok = lambda *a: emul("limit", *a)["status"]
    for kind in (IPA, SMSM):
        assert ok(kind, 1, 0) == 1 and ok(kind, 1, 3) == 1 and ok(kind, 1, 12) == 1 and ok(kind, 0, 6) == 1           # not a power of two
        assert ok(kind, 0, 8) == 0
    assert ok(IPA, 16384, 2) == 0 and ok(IPA, 16385, 2) == 2                       # 4 count <= 2^16 tasks
    assert ok(SMSM, 10922, 2) == 0 and ok(SMSM, 10923, 2) == 2                     # 6 count <= 2^16
    # count (2 n + 2) <= 2^24: n = 2^22 leaves 2^23 + 2 per item
    assert ok(IPA, 1, 1 << 22) == 0 and ok(IPA, 2, 1 << 22) == 2 and ok(IPA, 1, 1 << 23) == 2
    assert (1 << 24) // 2050 == 8184 and ok(IPA, 8184, 1024) == 0 and ok(IPA, 8185, 1024) == 2
    # 3 count n <= 2^24
    assert ok(SMSM, 1, 1 << 22) == 0 and ok(SMSM, 2, 1 << 22) == 2 and ok(SMSM, 1, 1 << 23) == 2
    assert ok(SMSM, 5461, 1024) == 0 and ok(SMSM, 5462, 1024) == 2                 # 2^24 / 3072 = 5461.3
    assert ok(IPA, 1 << 60, 1 << 60) == 2 and ok(SMSM, 1 << 62, 2) == 2           # no wrap on the way to the limit


# ---- the reference model of the loop against the oracle's own provers ----
@pytest.mark.parametrize("kind", [IPA, SMSM], ids=["ipa", "same_msm"])
def test_the_python_loop_equals_the_oracles_prover_at_n_8(orc, kind):
    c = subarg_lib.case(kind, 20261020 + kind, 8, pad=2 if kind == SMSM else 0, filler=b"abc")
    m = subarg_lib.model_loop(orc, kind, 8, c["bases"], c["vecs"], c["state_in"])
    assert m["rounds"] == c["rounds"] and m["finals"] == c["finals"] and m["state"] == c["state_out"]
    assert len(m["rounds"]) == 3 * subarg_lib.TERMS[kind] * 48 and len(m["attempts"]) == 3
    # the serialised proof is the entry commitments, the rounds' points in the serialiser's order, the canonical finals
    t = subarg_lib.TERMS[kind]
    pts = [[c["rounds"][(j * t + q) * 48:(j * t + q + 1) * 48] for j in range(3)] for q in range(t)]
    order = (0, 2, 1, 3) if kind == IPA else range(6)                  # L_C R_C L_D R_D / L_A L_T L_U R_A R_T R_U
    assert c["proof"] == c["pre"] + b"".join(b"".join(pts[q]) for q in order) + orc.fr_to_canonical_bytes(c["finals"])
