"""A plain reference for the transcripts: Keccak-f[1600] on 25 Python integers (FIPS 202), STROBE-128 as Merlin 3.0.0 uses it (rate
166, the operations meta-AD, AD and PRF with the `more` flag) and, on top, the Curdleproofs transcript (append(label, Fr),
get_and_append_challenge).  Written from the specifications for readability, not speed; it depends on neither the product nor the
oracle.  tests/test_transcript_check_cpu.py pins it against the oracle's Keccak and Merlin.

Every object keeps a trace of what it did and where in the rate it did it, so that the tests can assert from the reference alone
which positions, boundary splits and retries a set of cases reaches:
  ("op", name, pos)              a caller-level operation `name` started at position `pos`
  ("header", pos)                the two header bytes of an operation were written from position `pos` (165: they straddle)
  ("bytes", kind, pos, n)        n bytes of kind "label" | "len" | "data" | "scalar" were absorbed from position `pos`
  ("attempt", accepted)          one attempt of a challenge
"""

MASK64 = (1 << 64) - 1
R_FR = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001   # the order of BLS12-381's scalar field
RATE = 166
FLAG_I, FLAG_A, FLAG_C, FLAG_T, FLAG_M, FLAG_K = 1, 2, 4, 8, 16, 32

# rho's rotation offsets, indexed x + 5 y, and the 24 round constants of iota (FIPS 202, 3.2.2 and 3.2.5)
RHO = [0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14]


def _round_constants():
    rc, lfsr = [], 1
    for _ in range(24):
        c = 0
        for j in range(7):
            if lfsr & 1:
                c |= 1 << ((1 << j) - 1)
            lfsr <<= 1
            if lfsr & 0x100:
                lfsr ^= 0x171
        rc.append(c)
    return rc


RC = _round_constants()


def rol64(x, s):
    s %= 64
    return ((x << s) | (x >> (64 - s))) & MASK64 if s else x


def keccak_f1600(a):
    """the permutation on 25 integers a[x + 5 y]; returns a new list"""
    a = list(a)
    for rnd in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]                       # theta
        d = [c[(x + 4) % 5] ^ rol64(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):                                                                                 # rho and pi
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rol64(a[x + 5 * y], RHO[x + 5 * y])
        a = [b[i] ^ (~b[(i % 5 + 1) % 5 + 5 * (i // 5)] & MASK64 & b[(i % 5 + 2) % 5 + 5 * (i // 5)]) for i in range(25)]   # chi
        a[0] ^= RC[rnd]                                                                                    # iota
    return a


def state_to_bytes(words):
    return b"".join(w.to_bytes(8, "little") for w in words)


def bytes_to_state(b):
    return [int.from_bytes(b[8 * i:8 * i + 8], "little") for i in range(25)]


class Strobe:
    """STROBE-128 over Keccak-f[1600], the subset Merlin uses.  `permute` maps 25 words to 25 words."""

    def __init__(self, permute=keccak_f1600):
        self.permute = permute
        self.st = bytearray(200)
        self.pos = self.pos_begin = 0
        self.trace = []

    @classmethod
    def new(cls, protocol_label, permute=keccak_f1600):
        s = cls(permute)
        s.st[0:6] = bytes([1, RATE + 2, 1, 0, 1, 96])
        s.st[6:18] = b"STROBEv1.0.2"
        s._permute()
        s.meta_ad(protocol_label, False)
        return s

    # ---- the 27-word form the product exports: 25 words, pos, pos_begin ----
    @classmethod
    def from_words(cls, w27, permute=keccak_f1600):
        s = cls(permute)
        s.st = bytearray(state_to_bytes(w27[:25]))
        s.pos, s.pos_begin = int(w27[25]), int(w27[26])
        return s

    def to_words(self):
        return bytes_to_state(bytes(self.st)) + [self.pos, self.pos_begin]

    def _permute(self):
        self.st = bytearray(state_to_bytes(self.permute(bytes_to_state(bytes(self.st)))))

    def _run_f(self):
        self.st[self.pos] ^= self.pos_begin
        self.st[self.pos + 1] ^= 0x04
        self.st[RATE + 1] ^= 0x80
        self._permute()
        self.pos = self.pos_begin = 0

    def _absorb(self, data):
        for b in data:
            self.st[self.pos] ^= b
            self.pos += 1
            if self.pos == RATE:
                self._run_f()

    def _squeeze(self, n):
        out = bytearray()
        for _ in range(n):
            out.append(self.st[self.pos])
            self.st[self.pos] = 0
            self.pos += 1
            if self.pos == RATE:
                self._run_f()
        return bytes(out)

    def _begin_op(self, flags, more):
        if more:
            return
        assert not flags & FLAG_T
        self.trace.append(("header", self.pos))
        old_begin = self.pos_begin
        self.pos_begin = self.pos + 1
        self._absorb(bytes([old_begin, flags]))
        if flags & (FLAG_C | FLAG_K) and self.pos != 0:
            self._run_f()

    def meta_ad(self, data, more, kind="label"):
        self._begin_op(FLAG_M | FLAG_A, more)
        self.trace.append(("bytes", kind, self.pos, len(data)))
        self._absorb(data)

    def ad(self, data, more, kind="data"):
        self._begin_op(FLAG_A, more)
        self.trace.append(("bytes", kind, self.pos, len(data)))
        self._absorb(data)

    def prf(self, n):
        self._begin_op(FLAG_I | FLAG_A | FLAG_C, False)
        return self._squeeze(n)


class Transcript:
    """merlin::Transcript and the two methods of the Curdleproofs transcript on top of it"""

    def __init__(self, label=None, permute=keccak_f1600, strobe=None):
        if strobe is not None:
            self.s = strobe
            return
        self.s = Strobe.new(b"Merlin v1.0", permute)
        self.append_message(b"dom-sep", label)

    @classmethod
    def from_words(cls, w27, permute=keccak_f1600):
        return cls(strobe=Strobe.from_words(w27, permute))

    def to_words(self):
        return self.s.to_words()

    @property
    def trace(self):
        return self.s.trace

    def _op(self, name):
        self.s.trace.append(("op", name, self.s.pos))

    # ---- merlin ----
    def append_begin(self, label, total, _traced=False):
        """append_message up to the data: the pieces follow through absorb()"""
        if not _traced:
            self._op("append_begin")
        self.s.meta_ad(label, False)
        self.s.meta_ad(total.to_bytes(4, "little"), True, kind="len")
        self.s.ad(b"", False)

    def absorb(self, data, kind="data"):
        self._op("absorb")
        self.s.ad(data, True, kind=kind)

    def append_message(self, label, data, _traced=False, kind="data"):
        if not _traced:
            self._op("append_message")
        self.append_begin(label, len(data), _traced=True)
        self.s.ad(data, True, kind=kind)

    def challenge_bytes(self, label, n):
        self.s.meta_ad(label, False)
        self.s.meta_ad(n.to_bytes(4, "little"), True, kind="len")
        return self.s.prf(n)

    def meta_ad(self, data, more):
        self._op("meta_ad_more" if more else "meta_ad")
        self.s.meta_ad(data, more, kind="len" if more else "label")

    # ---- CurdleproofsTranscript ----
    def append_scalar(self, label, x, _traced=False):
        """append(label, &Fr): the canonical 32 little-endian bytes"""
        if not _traced:
            self._op("append_scalar")
        assert 0 <= x < R_FR
        self.append_message(label, x.to_bytes(32, "little"), _traced=True, kind="scalar")

    def get_and_append_challenge(self, label):
        """64 PRF bytes, the first 32 with the top bit cleared read as an integer; accepted when canonical and non-zero, then
        appended back under the same label.  Returns (scalar, attempts)."""
        self._op("challenge_scalar")
        attempts = 0
        while True:
            attempts += 1
            if attempts > 1:
                self._op("challenge_retry")
            buf = bytearray(self.challenge_bytes(label, 64)[:32])
            buf[31] &= 0x7f
            x = int.from_bytes(buf, "little")
            ok = 0 < x < R_FR
            self.s.trace.append(("attempt", ok))
            if ok:
                self.append_scalar(label, x, _traced=True)
                return x, attempts


def to_mont(x):
    """the Montgomery form the product returns scalars in: x 2^256 mod r"""
    return (x << 256) % R_FR


# ---- reading a trace ----
def op_positions(trace):
    """the set of (operation, pos) pairs of a trace"""
    return {(e[1], e[2]) for e in trace if e[0] == "op"}


def splits(trace, kind):
    """for every run of `kind` bytes that a rate boundary cuts inside: (bytes before the first cut, length)"""
    out = []
    for e in trace:
        if e[0] == "bytes" and e[1] == kind:
            k = RATE - e[2]
            if 0 < k < e[3]:
                out.append((k, e[3]))
    return out


def ends(trace, kind="data"):
    """the position after the last byte of every non-empty run of `kind` bytes, 166 where it ends on the boundary"""
    return [(e[2] + e[3] - 1) % RATE + 1 for e in trace if e[0] == "bytes" and e[1] == kind and e[3]]
