"""Expected values for the tests of cpx_ipa_verify / cpx_same_msm_verify: tests/host_emul/subarg_verify_oracle.cpp, a shared library over
oracle/protocol.h.  `make` gives a seeded CONSISTENT statement with the oracle's own proof of it, `verify` the oracle's own ipa_verify /
samemsm_verify on whatever inputs the test hands it (a fresh transcript, a fresh accumulator, the given draws): verdict, challenges and
the state afterwards.  The library under test is never the source of an expected value.

The proof layout restated here (slots in byte order) is the reference's `serialize` (inner_product_argument.rs:328-338,
same_multiscalar_argument.rs:263-275); tests/test_subarg_verify_cpu.py checks curdleproofs_amd/csrc/subarg_check_plan.hpp against it."""
import ctypes

from tests import subarg_lib
from tests.check_harness import build_emul
from tests.subarg_lib import IPA, SMSM, R_

FR, AFF, JAC, ST = 32, 96, 144, 216
OK, ERR_VERIFY, ERR_DESERIALIZE = 0, -4, -5            # include/cpx.h CPX_OK, CPX_ERR_VERIFY, CPX_ERR_DESERIALIZE
CHECKS = {IPA: 2, SMSM: 3}                             # accumulate_check calls = random factors per item
FAMILIES = {IPA: 1, SMSM: 3}
FIRST = {IPA: 2, SMSM: 3}                              # B_c B_d / B_a B_t B_u come first
BLOCKS = {IPA: ("L_C", "R_C", "L_D", "R_D"), SMSM: ("L_A", "L_T", "L_U", "R_A", "R_T", "R_U")}   # L slots each, in byte order
ROUND_ORDER = {IPA: ("L_C", "L_D", "R_C", "R_D"), SMSM: BLOCKS[SMSM]}                           # as a round appends them

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = ["oracle/" + f for f in ("protocol.h", "merlin.h", "g1.h", "field.h", "stdrng.h")]
        _lib = ctypes.CDLL(build_emul("subarg_verify_oracle.cpp", deps, shared=True))
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        _lib.sv_make.argtypes = [ci, ctypes.c_uint64, sz, vp, sz] + [vp] * 5 + [ctypes.POINTER(sz)]
        _lib.sv_verify.argtypes = [ci, sz, vp, sz, vp, vp, vp, vp, vp, sz, vp, ctypes.POINTER(ci), vp, vp]
        _lib.sv_entry.argtypes = [ci, ctypes.c_uint64, sz, vp, sz] + [vp] * 4
        _lib.sv_serialized_len.argtypes = [ci, sz]
        _lib.sv_serialized_len.restype = sz
    return _lib


def log2(n):
    return n.bit_length() - 1


def proof_points(kind, L):
    return FIRST[kind] + len(BLOCKS[kind]) * L


def proof_bytes(kind, L):
    return 48 * proof_points(kind, L) + FR * (2 if kind == IPA else 1)


def n_challenges(kind, L):
    return (2 if kind == IPA else 1) + L


def slot(kind, L, name, j=0):
    """the index of a proof point in byte order: "B_c", "B_d" / "B_a", "B_t", "B_u", or a block name with the round j"""
    firsts = ("B_c", "B_d") if kind == IPA else ("B_a", "B_t", "B_u")
    if name in firsts:
        return firsts.index(name)
    return FIRST[kind] + BLOCKS[kind].index(name) * L + j


def point(proof, s):
    return proof[48 * s:48 * (s + 1)]


def with_point(proof, s, enc):
    assert len(enc) == 48
    return proof[:48 * s] + enc + proof[48 * (s + 1):]


def scalar_at(kind, L, i):
    return 48 * proof_points(kind, L) + FR * i


def scalar(kind, L, proof, i):
    o = scalar_at(kind, L, i)
    return int.from_bytes(proof[o:o + FR], "little")


def with_scalar(kind, L, proof, i, value):
    """value is written as it is (32 bytes little-endian), reduced or not"""
    o = scalar_at(kind, L, i)
    return proof[:o] + int(value).to_bytes(FR, "little") + proof[o + FR:]


_made = {}


def make(kind, seed, n, filler=b""):
    """one seeded consistent statement and the oracle's proof of it.  bases: (G,) or (G, T, U) affine wire bytes; stmt: (crs_H, C, D) or
    (A, Z_t, Z_u) Jacobian wire bytes; z, vec_u (IPA; empty otherwise) Montgomery wire bytes; state_in: the state before `verify`."""
    key = (kind, seed, n, filler)
    if key in _made:
        return dict(_made[key])
    L = log2(n)
    buf = lambda size: (ctypes.c_uint8 * max(size, 1))()
    bases, stmt, z, u, proof = buf(FAMILIES[kind] * n * AFF), buf(3 * JAC), buf(FR), buf(n * FR), buf(proof_bytes(kind, L))
    plen = ctypes.c_size_t(0)
    assert lib().sv_make(kind, seed, n, filler, len(filler), bases, stmt, z, u, proof, ctypes.byref(plen)) == 0
    assert plen.value == proof_bytes(kind, L)
    b, s = bytes(bases), bytes(stmt)
    c = dict(kind=kind, n=n, filler=filler, bases=tuple(b[n * AFF * f:n * AFF * (f + 1)] for f in range(FAMILIES[kind])),
             stmt=tuple(s[JAC * k:JAC * (k + 1)] for k in range(3)), z=bytes(z) if kind == IPA else b"", vec_u=bytes(u) if kind == IPA else b"",
             proof=bytes(proof)[:plen.value], state_in=subarg_lib.entry_state(filler))
    _made[key] = c
    return dict(c)


def verify(c, rand):
    """the oracle's verdict on item c (a dict as `make` returns, possibly changed by the test) with the draws `rand`:
    dict(verdict = OK / ERR_VERIFY / ERR_DESERIALIZE, challenges = wire bytes, state = 216 bytes)"""
    kind, n = c["kind"], c["n"]
    L = log2(n)
    assert len(rand) == CHECKS[kind] * FR
    verdict = ctypes.c_int(1)
    chal, state = (ctypes.c_uint8 * (n_challenges(kind, L) * FR))(), (ctypes.c_uint8 * ST)()
    bases = b"".join(c["bases"])
    rc = lib().sv_verify(kind, n, c["filler"], len(c["filler"]), bases, b"".join(c["stmt"]), c["z"] or None, c["vec_u"] or None, c["proof"], len(c["proof"]), rand,
                         ctypes.byref(verdict), chal, state)
    assert rc == 0, "the shim returned %d" % rc
    return dict(verdict=verdict.value, challenges=bytes(chal), state=bytes(state))


def loop_entry(kind, seed, n, filler=b""):
    """what stands at the entry of the prover's log-round loop for the statement make(kind, seed, n, filler) gives (n >= 2): the bases
    and vectors Context.ipa_rounds / same_msm_rounds take, the state, and the head of the proof (the B points, compressed)"""
    c = make(kind, seed, n, filler)
    buf = lambda size: (ctypes.c_uint8 * max(size, 1))()
    fam2, vecs, state, pre = buf((n + 1) * AFF), buf(2 * n * FR), buf(ST), buf(48 * FIRST[kind])
    assert lib().sv_entry(kind, seed, n, filler, len(filler), fam2, vecs, state, pre) == 0
    f, v = bytes(fam2), bytes(vecs)
    if kind == IPA:
        return dict(bases=(c["bases"][0], f[:n * AFF], f[n * AFF:(n + 1) * AFF]), vecs=(v[:n * FR], v[n * FR:2 * n * FR]), state=bytes(state), pre=bytes(pre))
    return dict(bases=c["bases"], vecs=(v[:n * FR],), state=bytes(state), pre=bytes(pre))


def serialized_len(kind, L):
    return lib().sv_serialized_len(kind, L)


def factors(orc, seed, kind, count=1):
    """count * CHECKS[kind] draws of Fr::rand, as wire bytes (non-zero with overwhelming probability; asserted)"""
    w = orc.rng(seed).fr(count * CHECKS[kind])
    assert all(w[FR * i:FR * (i + 1)] != bytes(FR) for i in range(count * CHECKS[kind]))
    return w


# ---- the flattened check restated on integers (subarg_check_plan.hpp says the same over Fr) ----
def model_row(kind, n, a, chal, fin, z=0, u=()):
    """the weights of an item's row of points: G [n] (| T [n] | U [n]) | the proof's points in byte order | crs_H C D resp. A Z_t Z_u.
    a: the random factors, chal: alpha, (beta,) gamma_1..L, fin: (c, d) or (x,) — all integers mod r"""
    L = log2(n)
    alpha = chal[0]
    gam = list(chal[2:] if kind == IPA else chal[1:])
    inv = [pow(g, R_ - 2, R_) for g in gam]
    assert len(gam) == L

    def s_of(i, g):
        r = 1
        for j in range(L):
            if (i >> (L - 1 - j)) & 1:
                r = r * g[j] % R_
        return r

    row = []
    if kind == IPA:
        beta, (cf, df) = chal[1], fin
        row += [(a[0] * cf * s_of(i, gam) + a[1] * df * u[i] * s_of(i, inv)) % R_ for i in range(n)]
    else:
        for k in range(3):
            row += [a[k] * fin[0] * s_of(i, gam) % R_ for i in range(n)]
    row += [-a[k] % R_ for k in range(CHECKS[kind])]
    for name in BLOCKS[kind]:
        k = ("C", "D").index(name[2]) if kind == IPA else ("A", "T", "U").index(name[2])
        row += [-a[k] * (gam if name[0] == "L" else inv)[j] % R_ for j in range(L)]
    if kind == IPA:
        row += [a[0] * beta * (cf * df - alpha * alpha * z) % R_]
    row += [-a[k] * alpha % R_ for k in range(CHECKS[kind])]
    return row


def mutations(orc, c):
    """every single change the tests make that leaves the bytes decodable: name -> the changed item"""
    kind, n = c["kind"], c["n"]
    L = log2(n)
    plus1 = lambda wire: subarg_lib.to_wire(orc, [subarg_lib.to_ints(orc, wire)[0] + 1])
    out = {}
    if kind == IPA:
        out["z + 1"] = dict(c, z=plus1(c["z"]))
        out["c_final + 1"] = dict(c, proof=with_scalar(kind, L, c["proof"], 0, (scalar(kind, L, c["proof"], 0) + 1) % R_))
        out["one vec_u entry"] = dict(c, vec_u=c["vec_u"][:FR * (n - 1)] + plus1(c["vec_u"][FR * (n - 1):]))
        other = orc.g1_compress(orc.rng(4242).g1_affine(1))
        if L:
            out["another L_D"] = dict(c, proof=with_point(c["proof"], slot(kind, L, "L_D", L - 1), other))
        left, right = "L_C", "R_C"
    else:
        out["x_final + 1"] = dict(c, proof=with_scalar(kind, L, c["proof"], 0, (scalar(kind, L, c["proof"], 0) + 1) % R_))
        out["B_t = B_u"] = dict(c, proof=with_point(c["proof"], slot(kind, L, "B_t"), point(c["proof"], slot(kind, L, "B_u"))))
        T = c["bases"][1]
        out["a base of T"] = dict(c, bases=(c["bases"][0], orc.rng(4343).g1_affine(1) + T[AFF:], c["bases"][2]))
        left, right = "L_T", "R_T"
    if L:
        sl, sr = slot(kind, L, left, 0), slot(kind, L, right, 0)
        p = with_point(with_point(c["proof"], sl, point(c["proof"], sr)), sr, point(c["proof"], sl))
        out["L and R swapped"] = dict(c, proof=p)
    return out


def model_transcript(orc, c):
    """the transcript side of `verify` restated on tests/strobe_ref.py, from c["state_in"]: (transcript with its trace, challenges as
    integers).  tests/test_subarg_verify_cpu.py pins it against the oracle; the GPU test reads the trace to choose entry states."""
    from tests import strobe_ref
    kind, n = c["kind"], c["n"]
    L = log2(n)
    t = strobe_ref.Transcript.from_words(subarg_lib.words(c["state_in"]))
    stmt = orc.g1_compress_jac(b"".join(c["stmt"]))
    pt = lambda name, j=0: point(c["proof"], slot(kind, L, name, j))
    chal = []
    if kind == IPA:
        step, loop, gamma = b"ipa_step1", b"ipa_loop", b"ipa_gamma"
        t.append_message(step, stmt[48:96])
        t.append_message(step, stmt[96:144])
        t.append_scalar(step, subarg_lib.to_ints(orc, c["z"])[0])
        t.append_message(step, pt("B_c"))
        t.append_message(step, pt("B_d"))
        chal += [t.get_and_append_challenge(b"ipa_alpha")[0], t.get_and_append_challenge(b"ipa_beta")[0]]
    else:
        step, loop, gamma = b"same_msm_step1", b"same_msm_loop", b"same_msm_gamma"
        for k in range(3):
            t.append_message(step, stmt[48 * k:48 * (k + 1)])
        for f in (1, 2):                                        # Vec<G1Affine>: the length as u64, then the encodings
            t.append_message(step, n.to_bytes(8, "little") + orc.g1_compress(c["bases"][f]))
        for name in ("B_a", "B_t", "B_u"):
            t.append_message(step, pt(name))
        chal.append(t.get_and_append_challenge(b"same_msm_alpha")[0])
    for j in range(L):
        for name in ROUND_ORDER[kind]:
            t.append_message(loop, pt(name, j))
        chal.append(t.get_and_append_challenge(gamma)[0])
    return t, chal
