"""The reference's `rng: &mut T` for the calls that draw on the device (include/cpx.h, "the reference's rng as a ChaCha12 state").

    rng = StdRng.seed_from_u64(0)             # rand 0.8 StdRng::seed_from_u64(0) = ChaCha12Rng
    k = rng.fr(ctx, 1)                        # Fr::rand(&mut rng), drawn by the device, rng advanced
    children = rng.split(count)               # ChaCha12Rng::from_rng(&mut rng), count times: one stream per item of a batch
    P = rng.g1(ctx, 1)                        # G1Projective::rand(&mut rng).into_affine()
    draws = instance_draws(ctx, children)     # README.md:85-95 per stream: permutation, k, vec_R, vec_S

A StdRng holds the 40-byte state (key[32] || word_pos u64 LE) and nothing else; the streams themselves live in the library
(curdleproofs_amd/csrc/rng.hpp).  A state is secret prover randomness: two equal states draw equal witnesses, so never copy one into two
items — split."""
import ctypes

from . import AFF, CPX_ERR_STATE, CPX_OK, CpxError, FR, load_library

STATE_BYTES = 40


class StdRng:
    def __init__(self, state):
        state = bytes(state)
        if len(state) != STATE_BYTES:
            raise ValueError("StdRng: a state is 40 bytes (key[32] || word_pos u64 LE)")
        self.state = state

    @classmethod
    def seed_from_u64(cls, seed):
        out = (ctypes.c_uint8 * STATE_BYTES)()
        rc = load_library().cpx_rng_from_u64(seed & ((1 << 64) - 1), out)
        if rc != CPX_OK:
            raise CpxError(rc, "cpx_rng_from_u64")
        return cls(bytes(out))

    @property
    def word_pos(self):
        return int.from_bytes(self.state[32:], "little")

    def split(self, count=1):
        """`count` children, each keyed by the next eight words of this stream, which advances (cpx_rng_split)"""
        parent = (ctypes.c_uint8 * STATE_BYTES).from_buffer_copy(self.state)
        out = (ctypes.c_uint8 * max(STATE_BYTES * count, 1))()
        rc = load_library().cpx_rng_split(parent, count, out)
        if rc != CPX_OK:
            raise CpxError(rc, "cpx_rng_split")
        self.state = bytes(parent)
        return [StdRng(bytes(out)[STATE_BYTES * i: STATE_BYTES * (i + 1)]) for i in range(count)]

    def fr(self, ctx, n=1):
        """Fr::rand n times (cpx_rng_fr): n * 32 bytes, Montgomery limbs"""
        (out,) = fr_many(ctx, [self], n)
        return out

    def g1(self, ctx, n=1, compressed=False):
        """G1Projective::rand(&mut rng).into_affine() n times (cpx_rng_g1): n * 96 bytes, or (those, n * 48 compressed bytes)"""
        if compressed:
            aff, comp = g1_many(ctx, [self], n, compressed=True)
            return aff[0], comp[0]
        return g1_many(ctx, [self], n)[0]


def fr_many(ctx, rngs, n_each):
    """Fr::rand n_each times from every stream of `rngs` in one call; every stream advances.  Returns one bytes object per stream."""
    count = len(rngs)
    states = (ctypes.c_uint8 * max(STATE_BYTES * count, 1)).from_buffer_copy(b"".join(r.state for r in rngs) or b"\0")
    out = (ctypes.c_uint8 * max(FR * n_each * count, 1))()
    ctx._check(ctx._L.cpx_rng_fr(ctx._h, count, states, n_each, out))
    store_states(rngs, states)
    blob = bytes(out)
    return [blob[FR * n_each * i: FR * n_each * (i + 1)] for i in range(count)]


def g1_many(ctx, rngs, n_each, compressed=False):
    """G1Projective::rand(rng).into_affine() n_each times from every stream of `rngs` in one call (cpx_rng_g1); every stream advances.
    Returns one bytes object of n_each * 96 bytes per stream, or (that list, the list of n_each * 48 compressed bytes per stream)."""
    count = len(rngs)
    states = load_states(rngs)
    out = (ctypes.c_uint8 * max(AFF * n_each * count, 1))()
    comp = (ctypes.c_uint8 * max(48 * n_each * count, 1))() if compressed else None
    ctx._check(ctx._L.cpx_rng_g1(ctx._h, count, states, n_each, out, comp))
    store_states(rngs, states)
    blob = bytes(out)
    aff = [blob[AFF * n_each * i: AFF * n_each * (i + 1)] for i in range(count)]
    if not compressed:
        return aff
    cb = bytes(comp)
    return aff, [cb[48 * n_each * i: 48 * n_each * (i + 1)] for i in range(count)]


def instance_draws(ctx, rngs):
    """The draws that open the reference's README example (README.md:85-95), per stream at ctx.ell: the shuffle of 0..ell, k = Fr::rand,
    vec_R and vec_S (ell G1 draws each), in that order (cpx_rng_instance_draws).  Returns one (perm, k, vec_R, vec_S) per stream."""
    count, ell = len(rngs), ctx.ell
    if ell is None:
        raise CpxError(CPX_ERR_STATE, "set_crs first")
    states = load_states(rngs)
    perm = (ctypes.c_uint32 * max(count * ell, 1))()
    k = (ctypes.c_uint8 * max(FR * count, 1))()
    vr, vs = (ctypes.c_uint8 * max(AFF * ell * count, 1))(), (ctypes.c_uint8 * max(AFF * ell * count, 1))()
    ctx._check(ctx._L.cpx_rng_instance_draws(ctx._h, count, states, perm, k, vr, vs))
    store_states(rngs, states)
    kb, rb, sb = bytes(k), bytes(vr), bytes(vs)
    row = AFF * ell
    return [(list(perm[ell * i: ell * (i + 1)]), kb[FR * i: FR * (i + 1)], rb[row * i: row * (i + 1)], sb[row * i: row * (i + 1)]) for i in range(count)]


def load_states(rngs):
    return (ctypes.c_uint8 * max(STATE_BYTES * len(rngs), 1)).from_buffer_copy(b"".join(r.state for r in rngs) or b"\0")


def store_states(rngs, states):
    blob = bytes(states)
    for i, r in enumerate(rngs):
        r.state = blob[STATE_BYTES * i: STATE_BYTES * (i + 1)]
