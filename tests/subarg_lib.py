"""Expected values for the tests of cpx_ipa_rounds / cpx_same_msm_rounds and of the cpx_transcript_* calls.

Two sources, neither of them the library under test:
  * tests/host_emul/subarg_oracle.cpp, a shared library over oracle/protocol.h: seeded inputs, the steps before the log-round loop with
    the oracle's primitives, what stands at loop entry, and the oracle's own ipa_new / samemsm_new on the same inputs (`case`);
  * a restatement of the loop itself in Python (`model_loop`): tests/strobe_ref.py for the transcript, the oracle's group calls for the
    points, integers for the scalars.  tests/test_loop_rounds_cpu.py pins it against ipa_new / samemsm_new; the GPU tests use it where
    the entry values are chosen by the test (zero halves, identity bases, filler that moves the rate position).
"""
import ctypes

from tests import strobe_ref
from tests.check_harness import build_emul

FR, AFF = 32, 96
R_ = strobe_ref.R_FR
IDENTITY48 = bytes([0xc0]) + bytes(47)
IPA, SMSM = 0, 1
TERMS = {IPA: 4, SMSM: 6}
LABELS = {IPA: (b"ipa_loop", b"ipa_gamma"), SMSM: (b"same_msm_loop", b"same_msm_gamma")}

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = ["oracle/" + f for f in ("protocol.h", "merlin.h", "g1.h", "field.h", "stdrng.h")]
        _lib = ctypes.CDLL(build_emul("subarg_oracle.cpp", deps, shared=True))
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        _lib.sub_state.argtypes = [vp, sz, vp]
        _lib.sub_state.restype = None
        _lib.sub_ipa.argtypes = [ctypes.c_uint64, sz, sz, vp, sz] + [vp] * 11 + [ctypes.POINTER(sz)]
        _lib.sub_samemsm.argtypes = [ctypes.c_uint64, sz, sz, vp, sz] + [vp] * 10 + [ctypes.POINTER(sz)]
    return _lib


def words(state):
    return [int.from_bytes(state[8 * i:8 * i + 8], "little") for i in range(27)]


def state_bytes(w27):
    return b"".join(int(w).to_bytes(8, "little") for w in w27)


def entry_state(filler=b""):
    """Transcript::new("subarg") + one message of the filler under "filler" (none when empty), as the oracle's Merlin leaves it"""
    out = (ctypes.c_uint8 * 216)()
    lib().sub_state(filler, len(filler), out)
    return bytes(out)


def case(kind, seed, n, pad=0, filler=b""):
    """one seeded stand-alone proof: dict of the loop's entry values (bases, H, vectors, state_in) and the oracle's results"""
    L = n.bit_length() - 1
    buf = lambda size: (ctypes.c_uint8 * max(size, 1))()
    plen = ctypes.c_size_t(0)
    st_in, st_out = buf(216), buf(216)
    rounds, proof = buf(L * TERMS[kind] * 48), buf((3 + 6 * L) * 48 + 64)
    if kind == IPA:
        G, Gp, H, c, d, pre, fin = buf(n * AFF), buf(n * AFF), buf(AFF), buf(n * FR), buf(n * FR), buf(96), buf(64)
        rc = lib().sub_ipa(seed, n, pad, filler, len(filler), G, Gp, H, c, d, st_in, pre, rounds, fin, st_out, proof, ctypes.byref(plen))
        assert rc == 0
        return dict(kind=kind, n=n, bases=(bytes(G), bytes(Gp), bytes(H)), vecs=(bytes(c), bytes(d)), state_in=bytes(st_in), pre=bytes(pre), rounds=bytes(rounds),
                    finals=bytes(fin), state_out=bytes(st_out), proof=bytes(proof)[:plen.value])
    G, T, U, x, pre, fin = buf(n * AFF), buf(n * AFF), buf(n * AFF), buf(n * FR), buf(144), buf(32)
    rc = lib().sub_samemsm(seed, n, pad, filler, len(filler), G, T, U, x, st_in, pre, rounds, fin, st_out, proof, ctypes.byref(plen))
    assert rc == 0
    return dict(kind=kind, n=n, bases=(bytes(G), bytes(T), bytes(U)), vecs=(bytes(x),), state_in=bytes(st_in), pre=bytes(pre), rounds=bytes(rounds),
                finals=bytes(fin), state_out=bytes(st_out), proof=bytes(proof)[:plen.value])


# ---- the loop restated ----
def to_ints(orc, wire):
    b = orc.fr_to_canonical_bytes(wire)
    return [int.from_bytes(b[FR * i:FR * (i + 1)], "little") for i in range(len(wire) // FR)]


def to_wire(orc, ints):
    return orc.fr_from_canonical_bytes(b"".join((v % R_).to_bytes(32, "little") for v in ints)) if ints else b""


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b)) % R_


def round_transcript(kind, state, encodings):
    """the transcript side of ONE round alone: the round's encodings appended, the challenge drawn.  Returns (transcript, gamma, attempts):
    what a search over entry states needs, without a group operation"""
    loop_label, gamma_label = LABELS[kind]
    t = strobe_ref.Transcript.from_words(words(state))
    for q in range(TERMS[kind]):
        t.append_message(loop_label, encodings[48 * q:48 * (q + 1)])
    g, tries = t.get_and_append_challenge(gamma_label)
    return t, g, tries


def model_loop(orc, kind, n, bases, vecs, state):
    """inner_product_argument.rs:150-186 / same_multiscalar_argument.rs:99-136 with folded bases, as the reference writes them.
    bases: (G, G', H) or (G, T, U) wire bytes; vecs: (c, d) or (x,) wire bytes; state: 216 bytes.
    Returns dict(rounds = 48-byte encodings round after round, finals = wire bytes, gammas = wire bytes, state = 216 bytes,
    attempts = per round the attempts of the challenge, trace = the transcript's trace)."""
    loop_label, gamma_label = LABELS[kind]
    t = strobe_ref.Transcript.from_words(words(state))
    v = [to_ints(orc, w) for w in vecs]
    fams = [bytearray(b) for b in (bases[:2] if kind == IPA else bases)]
    H = bases[2] if kind == IPA else None
    rounds, gammas, attempts = b"", [], []
    m = n
    while m > 1:
        m //= 2
        left = lambda f: bytes(fams[f][:AFF * m])
        right = lambda f: bytes(fams[f][AFF * m:2 * AFF * m])
        if kind == IPA:
            c, d = v
            c_L, c_R, d_L, d_R = c[:m], c[m:2 * m], d[:m], d[m:2 * m]
            terms = [(right(0) + H, c_L + [_dot(c_L, d_R)]), (left(1), d_R), (left(0) + H, c_R + [_dot(c_R, d_L)]), (right(1), d_L)]
        else:
            x = v[0]
            x_L, x_R = x[:m], x[m:2 * m]
            terms = [(right(f), x_L) for f in range(3)] + [(left(f), x_R) for f in range(3)]
        for pts, sc in terms:
            enc = orc.g1_compress_jac(orc.g1_msm(pts, to_wire(orc, sc)))
            rounds += enc
            t.append_message(loop_label, enc)
        g, tries = t.get_and_append_challenge(gamma_label)
        gi = pow(g, R_ - 2, R_)
        gammas.append(g)
        attempts.append(tries)
        gw, giw = to_wire(orc, [g]), to_wire(orc, [gi])
        if kind == IPA:
            v[0] = [(c_L[i] + gi * c_R[i]) % R_ for i in range(m)]
            v[1] = [(d_L[i] + g * d_R[i]) % R_ for i in range(m)]
            fams[0] = bytearray(orc.g1_fold(left(0), right(0), gw))
            fams[1] = bytearray(orc.g1_fold(left(1), right(1), giw))
        else:
            v[0] = [(x_L[i] + gi * x_R[i]) % R_ for i in range(m)]
            for f in range(3):
                fams[f] = bytearray(orc.g1_fold(left(f), right(f), gw))
    return dict(rounds=rounds, finals=to_wire(orc, [w[0] for w in v]), gammas=to_wire(orc, gammas), state=state_bytes(t.to_words()), attempts=attempts,
                trace=t.trace)
