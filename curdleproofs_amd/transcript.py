"""merlin::Transcript with the crate's CurdleproofsTranscript (transcript.rs:14-60) as a value: the 216-byte state that crosses the C ABI
(include/cpx.h cpx_transcript_*) and that Context.ipa_rounds / Context.same_msm_rounds take at loop entry and hand back advanced.

    t = Transcript.new(b"curdleproofs")
    t.append_message(b"ipa_step1", compressed_point)
    alpha = t.challenge_scalar(b"ipa_alpha")            # 32 bytes, Montgomery limbs as everywhere in this package
    out = ctx.ipa_rounds(n, G, G_prime, H, c, d, t.state)
    t = Transcript.from_state(out["states"])

Host only: no context and no GPU are needed.  The operations are the library's (strobe.hpp), not a Python restatement."""
import ctypes

from . import CPX_OK, FR, TRANSCRIPT_BYTES, CpxError, load_library


def _label(label):
    return label.encode() if isinstance(label, str) else bytes(label)


class Transcript:
    def __init__(self, state):
        state = bytes(state)
        if len(state) != TRANSCRIPT_BYTES:
            raise ValueError("a transcript state is %d bytes" % TRANSCRIPT_BYTES)
        self._s = (ctypes.c_uint8 * TRANSCRIPT_BYTES).from_buffer_copy(state)
        self._L = load_library()

    @classmethod
    def new(cls, label):
        """merlin::Transcript::new(label)"""
        label = _label(label)
        out = (ctypes.c_uint8 * TRANSCRIPT_BYTES)()
        rc = load_library().cpx_transcript_new(label, len(label), out)
        if rc != CPX_OK:
            raise CpxError(rc, "cpx_transcript_new")
        return cls(bytes(out))

    @classmethod
    def from_state(cls, state):
        """a transcript that continues from a 216-byte state (one item's slice of what a loop call returned)"""
        return cls(state)

    @property
    def state(self):
        return bytes(self._s)

    def _check(self, rc, what):
        if rc != CPX_OK:
            raise CpxError(rc, what)

    def append_message(self, label, message):
        label, message = _label(label), bytes(message)
        self._check(self._L.cpx_transcript_append_message(self._s, label, len(label), message, len(message)), "cpx_transcript_append_message")

    def append_scalar(self, label, scalar):
        """transcript.rs:29-33 on an Fr (32 bytes, Montgomery limbs)"""
        label, scalar = _label(label), bytes(scalar)
        if len(scalar) != FR:
            raise ValueError("a scalar is 32 bytes")
        self._check(self._L.cpx_transcript_append_scalar(self._s, label, len(label), scalar), "cpx_transcript_append_scalar")

    def challenge_bytes(self, label, n):
        label = _label(label)
        out = (ctypes.c_uint8 * max(n, 1))()
        self._check(self._L.cpx_transcript_challenge_bytes(self._s, label, len(label), out, n), "cpx_transcript_challenge_bytes")
        return bytes(out)[:n]

    def challenge_scalar(self, label):
        """transcript.rs:41-54 get_and_append_challenge: retried until canonical and non-zero, appended back; Montgomery limbs"""
        label = _label(label)
        out = (ctypes.c_uint8 * FR)()
        self._check(self._L.cpx_transcript_challenge_scalar(self._s, label, len(label), out), "cpx_transcript_challenge_scalar")
        return bytes(out)
