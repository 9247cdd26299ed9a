"""Expected values for the tests of cpx_ipa_prove / cpx_same_msm_prove: tests/host_emul/subarg_prove_oracle.cpp, a shared library over
oracle/protocol.h.  `sp_inputs` makes seeded inputs (arbitrary as tests/subarg_lib.py `case` draws them, or consistent with the witness
exported), `sp_prove` runs the oracle's own ipa_new / samemsm_new on whatever inputs and draws the test hands it.  The library under test
is never the source of an expected value.

`model_blinders` restates generate_ipa_blinders (inner_product_argument.rs:42-82) on Python integers, `model_step1` the transcript of
step 1 on tests/strobe_ref.py (for the choice of entry states)."""
import ctypes

from tests import subarg_lib
from tests.check_harness import build_emul
from tests.subarg_lib import IPA, SMSM, R_
from tests.subarg_verify_lib import FR, AFF, JAC, ST, log2, n_challenges, proof_bytes

RNG_XOR = 0x9e3779b97f4a7c15     # the prover's stream of subarg_oracle.cpp: StdRng(seed ^ RNG_XOR)
FAMILIES = {IPA: 2, SMSM: 3}     # G | G'  resp.  G | T | U
NVEC = {IPA: 2, SMSM: 1}

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = ["oracle/" + f for f in ("protocol.h", "merlin.h", "g1.h", "field.h", "stdrng.h")]
        _lib = ctypes.CDLL(build_emul("subarg_prove_oracle.cpp", deps, shared=True))
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        _lib.sp_inputs.argtypes = [ci, ctypes.c_uint64, sz, ci, sz] + [vp] * 5
        _lib.sp_prove.argtypes = [ci, sz, vp, sz, vp, vp, vp, vp, vp, sz, vp, ctypes.POINTER(sz), vp, vp, ctypes.POINTER(ci)]
    return _lib


def draws_each(kind, n):
    return 2 * n - 2 if kind == IPA else n


_made = {}


def sp_inputs(kind, seed, n, consistent=False, pad=0, filler=b""):
    """one seeded item: dict(kind, n, filler, bases = (G, G') or (G, T, U) affine wire bytes, stmt = (crs_H, C, D) or (A, Z_t, Z_u)
    Jacobian wire bytes, z (IPA) and vecs = (c, d) or (x,) Montgomery wire bytes, vec_u (IPA, consistent: G' = u o G), state_in)"""
    key = (kind, seed, n, bool(consistent), pad, filler)
    if key in _made:
        return dict(_made[key])
    buf = lambda size: (ctypes.c_uint8 * max(size, 1))()
    bases, stmt, z, vecs, u = buf(FAMILIES[kind] * n * AFF), buf(3 * JAC), buf(FR), buf(NVEC[kind] * n * FR), buf(n * FR)
    assert lib().sp_inputs(kind, seed, n, 1 if consistent else 0, pad, bases, stmt, z, vecs, u) == 0
    b, s, v = bytes(bases), bytes(stmt), bytes(vecs)
    c = dict(kind=kind, n=n, filler=filler, bases=tuple(b[n * AFF * f:n * AFF * (f + 1)] for f in range(FAMILIES[kind])),
             stmt=tuple(s[JAC * k:JAC * (k + 1)] for k in range(3)), z=bytes(z) if kind == IPA else b"",
             vecs=tuple(v[n * FR * k:n * FR * (k + 1)] for k in range(NVEC[kind])), vec_u=bytes(u) if kind == IPA else b"",
             state_in=subarg_lib.entry_state(filler))
    _made[key] = c
    return dict(c)


def sp_prove(c, draws):
    """the oracle's own `new` on item c (a dict as sp_inputs returns, possibly changed by the test) with `draws` (wire bytes):
    dict(ok = False where the reference panics in generate_ipa_blinders, proof, challenges = wire bytes, state = 216 bytes)"""
    kind, n = c["kind"], c["n"]
    L = log2(n)
    assert len(draws) == draws_each(kind, n) * FR
    proof, chal, state = (ctypes.c_uint8 * proof_bytes(kind, L))(), (ctypes.c_uint8 * (n_challenges(kind, L) * FR))(), (ctypes.c_uint8 * ST)()
    plen, status = ctypes.c_size_t(0), ctypes.c_int(-1)
    rc = lib().sp_prove(kind, n, c["filler"], len(c["filler"]), b"".join(c["bases"]), b"".join(c["stmt"]), c["z"] or None, b"".join(c["vecs"]), draws or None,
                        len(draws) // FR, proof, ctypes.byref(plen), chal, state, ctypes.byref(status))
    assert rc == 0, "the shim returned %d" % rc
    assert plen.value == proof_bytes(kind, L)
    return dict(ok=status.value == 0, proof=bytes(proof), challenges=bytes(chal), state=bytes(state))


def seeded_draws(orc, kind, seed, n):
    """the draws subarg_oracle.cpp's provers make for `seed`"""
    return orc.rng(seed ^ RNG_XOR).fr(draws_each(kind, n)) if draws_each(kind, n) else b""


# ---- generate_ipa_blinders on integers ----
def model_blinders(c, d, r, z):
    """c, d, r of n integers, z of n - 2: (r_d = z with the two solved entries, or None where an inverse does not exist)"""
    n = len(c)
    assert len(d) == n and len(r) == n and len(z) == n - 2
    omega = (sum(a * b for a, b in zip(r, d)) + sum(a * b for a, b in zip(z, c[:n - 2]))) % R_
    delta = sum(a * b for a, b in zip(r[:n - 2], z)) % R_
    if c[n - 2] % R_ == 0:
        return None
    inv_c = pow(c[n - 2], R_ - 2, R_)
    den = (-r[n - 2] * inv_c * c[n - 1] + r[n - 1]) % R_
    if den == 0:
        return None
    last = (r[n - 2] * inv_c * omega - delta) * pow(den, R_ - 2, R_) % R_
    pen = -inv_c * (last * c[n - 1] + omega) % R_
    return list(z) + [pen, last]


def model_step1(orc, c, first):
    """step 1 of `new` restated on tests/strobe_ref.py from c["state_in"]; first: the B points' encodings (any 48-byte strings do for
    a search over rate positions).  Returns the transcript with its trace, before the first challenge is drawn."""
    from tests import strobe_ref
    kind, n = c["kind"], c["n"]
    t = strobe_ref.Transcript.from_words(subarg_lib.words(c["state_in"]))
    stmt = orc.g1_compress_jac(b"".join(c["stmt"]))
    if kind == IPA:
        step = b"ipa_step1"
        t.append_message(step, stmt[48:96])
        t.append_message(step, stmt[96:144])
        t.append_scalar(step, subarg_lib.to_ints(orc, c["z"])[0])
    else:
        step = b"same_msm_step1"
        for k in range(3):
            t.append_message(step, stmt[48 * k:48 * (k + 1)])
        for f in (1, 2):
            t.append_message(step, n.to_bytes(8, "little") + orc.g1_compress(c["bases"][f]))
    for k in range(len(first) // 48):
        t.append_message(step, first[48 * k:48 * (k + 1)])
    return t
