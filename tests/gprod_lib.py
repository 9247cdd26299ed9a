"""Expected values for the tests of cpx_gprod_prove: tests/host_emul/gprod_oracle.cpp, a shared library over oracle/protocol.h.
`gp_inputs` makes seeded inputs (consistent as grand_product_argument.rs:275-298 makes them, or arbitrary), `gp_prove` runs the oracle's
own gprod_new on whatever inputs and draws the test hands it, `gp_verify` its gprod_verify, `gp_derive` says what `new` hands the
inner-product prover.  The library under test is never the source of an expected value.

`PlanModel` restates curdleproofs_amd/csrc/gprod_plan.hpp on Python integers, `model_*` the algebra of gprod_algebra.hpp, `model_steps`
the transcript of steps 1 and 2 on tests/strobe_ref.py (for the choice of entry states)."""
import ctypes

from tests import subarg_lib
from tests.check_harness import build_emul
from tests.subarg_lib import R_

FR, AFF, JAC, ST = 32, 96, 144, 216
THREADS = 128                    # GPROD_THREADS of curdleproofs_amd/csrc/kernels.h

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = ["oracle/" + f for f in ("protocol.h", "merlin.h", "g1.h", "field.h", "stdrng.h")]
        _lib = ctypes.CDLL(build_emul("gprod_oracle.cpp", deps, shared=True))
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        _lib.gp_inputs.argtypes = [ctypes.c_uint64, sz, sz, ci] + [vp] * 9
        _lib.gp_derive.argtypes = [sz, sz, vp, sz] + [vp] * 13
        _lib.gp_prove.argtypes = [sz, sz, vp, sz] + [vp] * 8 + [sz, vp, ctypes.POINTER(sz), vp, vp, ctypes.POINTER(ci)]
        _lib.gp_inner.argtypes = [sz, sz, vp, sz] + [vp] * 10
        _lib.gp_verify.argtypes = [sz, sz, vp, sz] + [vp] * 8 + [sz, vp, vp]
    return _lib


def log2(n):
    return max(n.bit_length() - 1, 0)


def proof_bytes(L):
    return 48 * (3 + 4 * L) + 96


def n_challenges(L):
    return 4 + L


def draws_each(ell, nb):
    return nb + 2 * (ell + nb) - 2


_buf = lambda size: (ctypes.c_uint8 * max(size, 1))()
_made = {}


def gp_inputs(seed, ell, nb, consistent=True, filler=b""):
    """one seeded item: dict(ell, nb, filler, G, H affine wire bytes, crs_U, B Jacobian wire bytes, result, b, rb Montgomery wire bytes,
    g_sum, h_sum affine wire bytes, state_in)"""
    key = (seed, ell, nb, bool(consistent), filler)
    if key not in _made:
        G, H, U, B, res, b, rb, gs, hs = _buf(ell * AFF), _buf(nb * AFF), _buf(JAC), _buf(JAC), _buf(FR), _buf(ell * FR), _buf(nb * FR), _buf(AFF), _buf(AFF)
        assert lib().gp_inputs(seed, ell, nb, 1 if consistent else 0, G, H, U, B, res, b, rb, gs, hs) == 0
        _made[key] = dict(ell=ell, nb=nb, filler=filler, G=bytes(G)[:ell * AFF], H=bytes(H)[:nb * AFF], crs_U=bytes(U), B=bytes(B), result=bytes(res),
                          b=bytes(b)[:ell * FR], rb=bytes(rb)[:nb * FR], g_sum=bytes(gs), h_sum=bytes(hs), state_in=subarg_lib.entry_state(filler))
    return dict(_made[key])


def _args(c):
    return (c["ell"], c["nb"], c["filler"], len(c["filler"]), c["G"], c["H"] or None, c["crs_U"])


def gp_prove(c, draws):
    """the oracle's own `new` on item c (a dict as gp_inputs returns, possibly changed by the test) with `draws` (wire bytes):
    dict(ok = False where the reference panics in generate_ipa_blinders, proof, challenges = wire bytes, state = 216 bytes)"""
    ell, nb = c["ell"], c["nb"]
    L = log2(ell + nb)
    assert len(draws) == draws_each(ell, nb) * FR
    proof, chal, state = _buf(proof_bytes(L)), _buf(n_challenges(L) * FR), _buf(ST)
    plen, status = ctypes.c_size_t(0), ctypes.c_int(-1)
    rc = lib().gp_prove(*_args(c), c["B"], c["result"], c["b"], c["rb"] or None, draws, len(draws) // FR, proof, ctypes.byref(plen), chal, state, ctypes.byref(status))
    assert rc == 0, "the shim returned %d" % rc
    assert plen.value == proof_bytes(L)
    return dict(ok=status.value == 0, proof=bytes(proof), challenges=bytes(chal), state=bytes(state))


def gp_verify(c, proof, factors):
    """the oracle's `verify` of `proof` on item c's statement: dict(verdict = True, False or "deserialize", state)"""
    state = _buf(ST)
    rc = lib().gp_verify(*_args(c), c["g_sum"], c["h_sum"], c["B"], c["result"], proof, len(proof), factors, state)
    assert rc in (0, 1, 2), "the shim returned %d" % rc
    return dict(verdict={0: True, 1: False, 2: "deserialize"}[rc], state=bytes(state))


def gp_derive(c, c_blinders):
    """what `new` hands InnerProductProof::new: dict(n, bases = (G | H, G'), stmt = (crs_U, C, D), z, vecs = (c, d), state = after step 2)"""
    ell, nb = c["ell"], c["nb"]
    n = ell + nb
    bases, stmt, z, vecs, state = _buf(2 * n * AFF), _buf(3 * JAC), _buf(FR), _buf(2 * n * FR), _buf(ST)
    assert lib().gp_derive(*_args(c), c["B"], c["result"], c["b"], c["rb"] or None, c_blinders or None, bases, stmt, z, vecs, state) == 0
    b, s, v = bytes(bases), bytes(stmt), bytes(vecs)
    return dict(n=n, bases=(b[:n * AFF], b[n * AFF:]), stmt=tuple(s[JAC * k:JAC * (k + 1)] for k in range(3)), z=bytes(z), vecs=(v[:n * FR], v[n * FR:]),
                state=bytes(state))


def gp_inner(c, draws):
    """the oracle's ipa_new on what gp_derive exports, from the state after step 2, with the item's draws behind vec_c_blinders:
    dict(proof = the InnerProductProof bytes, state)"""
    L = log2(c["ell"] + c["nb"])
    out, state = _buf(proof_bytes(L) - 80), _buf(ST)
    assert lib().gp_inner(*_args(c), c["B"], c["result"], c["b"], c["rb"] or None, draws, out, state) == 0
    return dict(proof=bytes(out), state=bytes(state))


def seeded_draws(orc, seed, ell, nb):
    return orc.rng(seed ^ 0x5bd1e995).fr(draws_each(ell, nb))


# ---- gprod_algebra.hpp on integers ----
def inv(x):
    return pow(x % R_, R_ - 2, R_)


def model_products(b):
    """vec_c of grand_product_argument.rs:69-73: 1, b_0, b_0 b_1, ... (len(b) entries)"""
    out, run = [], 1
    for x in b:
        out.append(run)
        run = run * x % R_
    return out


def model_layer(b, rb, c_blinders, result, alpha, beta):
    """dict(r_p, u, d, d_scalars, inner_prod) of :79-142 for given challenges"""
    ell, nb = len(b), len(rb)
    bi = inv(beta)
    r_p = sum((x + alpha) * y for x, y in zip(rb, c_blinders)) % R_
    u = [pow(bi, i + 1, R_) for i in range(ell)] + [pow(bi, ell + 1, R_)] * nb
    d = [(b[i] * pow(beta, i + 1, R_) - pow(beta, i, R_)) % R_ for i in range(ell)] + [pow(beta, ell + 1, R_) * (x + alpha) % R_ for x in rb]
    return dict(r_p=r_p, u=u, d=d, d_scalars=[-bi % R_] * ell + [alpha % R_] * nb,
                inner_prod=(r_p * pow(beta, ell + 1, R_) + result * pow(beta, ell, R_) - 1) % R_)


# ---- gprod_plan.hpp on integers ----
class PlanModel:
    """the regions of curdleproofs_amd/csrc/gprod_plan.hpp behind those of subarg_prove_plan.hpp (IPA) and loop_plan.hpp, said again"""

    def __init__(self, count, ell, nb):
        n = ell + nb
        L = log2(n)
        self.count, self.ell, self.nb, self.n, self.L = count, ell, nb, n, L
        loop_fr = count * 4 * n + count * (2 * n + 2) + count + count * L + count * 2          # vectors | rows | ones | gammas | finals
        results = L * count * 4
        self.fr_wit = loop_fr
        self.fr_draws = self.fr_wit + count * 2 * n
        self.fr_rd = self.fr_draws + count * (2 * n - 2)
        self.fr_z = self.fr_rd + count * n
        self.fr_ab = self.fr_z + count
        sp_fr = self.fr_ab + 2 * count
        sp_points = count * 5
        names = ("result", "b", "rb", "cbl", "u", "dsc", "rdu", "rp", "chal")
        sizes = (count, count * ell, count * nb, count * nb, count * n, count * n, count * n, count, 2 * count)
        self.fr = {}
        at = sp_fr
        for name, size in zip(names, sizes):
            self.fr[name] = (at, size)
            at += size
        self.fr_total = at
        self.pt_B0 = sp_points
        self.jac_total = sp_points + count
        self.aff_total = results + sp_points + count
        sp_by = results * 48 + sp_points * 48 + count * 40
        self.by_B, self.by_C, self.by_total = sp_by, sp_by + 48 * count, sp_by + 96 * count
        self.ix_addend = 2 * L * (n // 2 + 1)
        self.ix_total = self.ix_addend + sp_points
        self.task_C = L * count * 4 + 2 * count
        self.task_D = self.task_C + count
        self.task_total = self.task_D + count
        self.proof_bytes = proof_bytes(L)
        self.draws_each = draws_each(ell, nb)
        self.challenges = n_challenges(L)
        self.addend = [0xffffffff] * sp_points
        for i in range(count):
            self.addend[2 * count + 3 * i + 2] = sp_points + i


def model_steps(orc, c, c_enc=bytes(48), r_p=0):
    """steps 1 and 2 of `new` restated on tests/strobe_ref.py from c["state_in"]; c_enc, r_p: any values do for a search over rate
    positions.  Returns the transcript with its trace, before beta is drawn."""
    from tests import strobe_ref
    t = strobe_ref.Transcript.from_words(subarg_lib.words(c["state_in"]))
    t.append_message(b"gprod_step1", orc.g1_compress_jac(c["B"]))
    t.append_scalar(b"gprod_step1", subarg_lib.to_ints(orc, c["result"])[0])
    t.get_and_append_challenge(b"gprod_alpha")
    t.append_message(b"gprod_step2", c_enc)
    t.append_scalar(b"gprod_step2", r_p)
    return t
