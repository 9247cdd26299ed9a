"""Expected values for the tests of cpx_same_perm_prove / cpx_same_perm_verify: tests/host_emul/same_perm_oracle.cpp, a shared library over
oracle/protocol.h.  `sp_inputs` makes seeded inputs (consistent as same_permutation_argument.rs:216-240 makes them, or arbitrary),
`sp_prove` runs the oracle's own sameperm_new on whatever inputs and draws the test hands it, `sp_verify` its sameperm_verify, `sp_derive`
says what `new` hands the grand-product prover, `sp_gprod` runs the oracle's gprod_new from a transcript state.  The library under test is
never the source of an expected value.

`model_step1` restates step 1 of the transcript on tests/strobe_ref.py, `model_weights` the extra relation's weights of
curdleproofs_amd/csrc/same_perm_algebra.hpp on integers."""
import ctypes
import struct

from tests import gprod_lib, subarg_lib
from tests.check_harness import build_emul
from tests.subarg_lib import R_

FR, AFF, JAC, ST = 32, 96, 144, 216
THREADS = gprod_lib.THREADS
PIECE = 128                      # SAME_PERM_PIECE of curdleproofs_amd/csrc/same_perm_plan.hpp
FIELDS = ("G", "H", "crs_U", "A", "M", "a", "perm", "ra", "rm")

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = ["oracle/" + f for f in ("protocol.h", "merlin.h", "g1.h", "field.h", "stdrng.h")] + ["tests/host_emul/gprod_oracle.cpp"]
        _lib = ctypes.CDLL(build_emul("same_perm_oracle.cpp", deps, shared=True))
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        _lib.sp_inputs.argtypes = [ctypes.c_uint64, sz, sz, ci] + [vp] * 11
        _lib.sp_derive.argtypes = [sz, sz] + [vp] * 14
        _lib.sp_gprod.argtypes = [sz, sz] + [vp] * 9 + [sz, vp, vp]
        _lib.sp_prove.argtypes = [sz, sz] + [vp] * 11 + [sz, vp, ctypes.POINTER(sz), vp, vp, ctypes.POINTER(ci)]
        _lib.sp_verify.argtypes = [sz, sz] + [vp] * 10 + [sz, vp, vp]
    return _lib


log2 = gprod_lib.log2
draws_each = gprod_lib.draws_each


def proof_bytes(L):
    return 48 + gprod_lib.proof_bytes(L)


def n_challenges(L):
    return 2 + gprod_lib.n_challenges(L)


_buf = lambda size: (ctypes.c_uint8 * max(size, 1))()
_made = {}


def perm_bytes(perm):
    return struct.pack("<%dI" % len(perm), *perm)


def perm_list(b):
    return list(struct.unpack("<%dI" % (len(b) // 4), b))


def sp_inputs(seed, ell, nb, consistent=True, filler=b""):
    """one seeded item: dict(ell, nb, G, H affine wire bytes, crs_U, A, M Jacobian wire bytes, a, ra, rm Montgomery wire bytes,
    perm = little-endian u32 bytes, g_sum, h_sum affine wire bytes, state_in)"""
    key = (seed, ell, nb, bool(consistent), filler)
    if key not in _made:
        G, H, U, A, M, a, perm = _buf(ell * AFF), _buf(nb * AFF), _buf(JAC), _buf(JAC), _buf(JAC), _buf(ell * FR), _buf(ell * 4)
        ra, rm, gs, hs = _buf(nb * FR), _buf(nb * FR), _buf(AFF), _buf(AFF)
        assert lib().sp_inputs(seed, ell, nb, 1 if consistent else 0, G, H, U, A, M, a, perm, ra, rm, gs, hs) == 0
        _made[key] = dict(ell=ell, nb=nb, G=bytes(G)[:ell * AFF], H=bytes(H)[:nb * AFF], crs_U=bytes(U), A=bytes(A), M=bytes(M), a=bytes(a)[:ell * FR],
                          perm=bytes(perm)[:ell * 4], ra=bytes(ra)[:nb * FR], rm=bytes(rm)[:nb * FR], g_sum=bytes(gs), h_sum=bytes(hs),
                          state_in=subarg_lib.entry_state(filler))
    return dict(_made[key])


def sp_derive(c):
    """what `new` hands GrandProductProof::new: dict(B, result, b, rb, alpha, beta (wire bytes), state = after step 1)"""
    ell, nb = c["ell"], c["nb"]
    B, res, b, rb, chal, state = _buf(JAC), _buf(FR), _buf(ell * FR), _buf(nb * FR), _buf(2 * FR), _buf(ST)
    assert lib().sp_derive(ell, nb, c["state_in"], c["G"], c["A"], c["M"], c["a"], c["perm"], c["ra"] or None, c["rm"] or None, B, res, b, rb, chal, state) == 0
    return dict(B=bytes(B), result=bytes(res), b=bytes(b)[:ell * FR], rb=bytes(rb)[:nb * FR], alpha=bytes(chal)[:FR], beta=bytes(chal)[FR:], state=bytes(state))


def sp_gprod(c, state_in, B, result, b, rb, draws):
    """the oracle's gprod_new on c's bases from `state_in`: dict(proof, state)"""
    ell, nb = c["ell"], c["nb"]
    proof, state = _buf(gprod_lib.proof_bytes(log2(ell + nb))), _buf(ST)
    assert lib().sp_gprod(ell, nb, state_in, c["G"], c["H"] or None, c["crs_U"], B, result, b, rb or None, draws, len(draws) // FR, proof, state) == 0
    return dict(proof=bytes(proof), state=bytes(state))


def sp_prove(c, draws):
    """the oracle's own `new` on item c with `draws` (wire bytes): dict(ok = False where the reference panics in generate_ipa_blinders,
    proof, challenges = wire bytes, state = 216 bytes)"""
    ell, nb = c["ell"], c["nb"]
    L = log2(ell + nb)
    assert len(draws) == draws_each(ell, nb) * FR
    proof, chal, state = _buf(proof_bytes(L)), _buf(n_challenges(L) * FR), _buf(ST)
    plen, status = ctypes.c_size_t(0), ctypes.c_int(-1)
    rc = lib().sp_prove(ell, nb, c["state_in"], c["G"], c["H"] or None, c["crs_U"], c["A"], c["M"], c["a"], c["perm"], c["ra"] or None, c["rm"] or None, draws,
                        len(draws) // FR, proof, ctypes.byref(plen), chal, state, ctypes.byref(status))
    assert rc == 0, "the shim returned %d" % rc
    assert plen.value == proof_bytes(L)
    return dict(ok=status.value == 0, proof=bytes(proof), challenges=bytes(chal), state=bytes(state))


def sp_verify(c, proof, factors):
    """the oracle's `verify` of `proof` on item c's statement with three factors: dict(verdict = True, False or "deserialize", state)"""
    assert len(factors) == 3 * FR
    state = _buf(ST)
    rc = lib().sp_verify(c["ell"], c["nb"], c["state_in"], c["G"], c["H"] or None, c["crs_U"], c["g_sum"], c["h_sum"], c["A"], c["M"], c["a"], proof, len(proof),
                         factors, state)
    assert rc in (0, 1, 2), "the shim returned %d" % rc
    return dict(verdict={0: True, 1: False, 2: "deserialize"}[rc], state=bytes(state))


def seeded_draws(orc, seed, ell, nb):
    return orc.rng(seed ^ 0x2545f491).fr(draws_each(ell, nb))


def factors(orc, seed, count=1):
    """three draws of Fr::rand per item, as wire bytes"""
    w = orc.rng(seed).fr(3 * count)
    assert all(w[FR * i:FR * (i + 1)] != bytes(FR) for i in range(3 * count))
    return w


# ---- step 1 on tests/strobe_ref.py ----
def vec_a_message(a_ints):
    """vec_a as a Vec<Fr>: the u64 little-endian length, then the canonical scalars — ONE message of 8 + 32 ell bytes"""
    return len(a_ints).to_bytes(8, "little") + b"".join((v % R_).to_bytes(32, "little") for v in a_ints)


def model_step1(state_in, enc_A, enc_M, a_ints):
    """step 1 (same_permutation_argument.rs:60-63) from a 216-byte state: (transcript with its trace, alpha, beta)"""
    from tests import strobe_ref
    t = strobe_ref.Transcript.from_words(subarg_lib.words(state_in))
    t.append_message(b"same_perm_step1", enc_A)
    t.append_message(b"same_perm_step1", enc_M)
    t.append_message(b"same_perm_step1", vec_a_message(a_ints))
    alpha = t.get_and_append_challenge(b"same_perm_alpha")[0]
    beta = t.get_and_append_challenge(b"same_perm_beta")[0]
    return t, alpha, beta


# ---- same_perm_algebra.hpp on integers ----
def model_factors(a, perm, alpha, beta):
    return [(a[s] + s * alpha + beta) % R_ for s in perm]


def model_weights(a0, alpha, beta):
    """dict(g_add, B, A, M): the relation beta <1, G> - (B - A - alpha M) == O with the factor a0, in the convention of
    subarg_check_plan.hpp"""
    return dict(g_add=a0 * beta % R_, B=-a0 % R_, A=a0 % R_, M=a0 * alpha % R_)
