"""Pure-Python model of the reference's randomness source, for the tests of curdleproofs_amd/csrc/rng.hpp and k_rng_draw: rand 0.8 `StdRng`
(= ChaCha12Rng: 12 rounds, 64-bit block counter, zero stream id) as a word stream with a position that can be read and set, and the samplers the
reference draws from it (ark-ff `Fr::rand`, rand 0.8 `SliceRandom::shuffle` over `UniformInt<u32>::sample_single`).  Restated from the
algorithms, not from the product header; tests/test_rng_check_cpu.py pins it against the oracle's StdRng (oracle/stdrng.h), which reproduces
the reference's two known-answer tests.  Every sampler can report what it rejected, which tests/rng_cases.py searches for its cases."""
import struct

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
M32 = 0xffffffff
STATE_BYTES = 40
POS_LIMIT = (1 << 64) - (1 << 32)     # states at or beyond it are refused by the library


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & M32


def chacha12_block(key, counter):
    """key: 8 words; returns the 16 words of block `counter`"""
    s = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + list(key) + [counter & M32, (counter >> 32) & M32, 0, 0]
    x = list(s)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & M32
        x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & M32
        x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & M32
        x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & M32
        x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(6):
        qr(0, 4, 8, 12), qr(1, 5, 9, 13), qr(2, 6, 10, 14), qr(3, 7, 11, 15)
        qr(0, 5, 10, 15), qr(1, 6, 11, 12), qr(2, 7, 8, 13), qr(3, 4, 9, 14)
    return [(a + b) & M32 for a, b in zip(x, s)]


def key_from_u64(seed):
    """rand_core 0.6 SeedableRng::seed_from_u64: eight PCG32 (XSH RR) outputs"""
    state, key = seed & ((1 << 64) - 1), []
    for _ in range(8):
        state = (state * 6364136223846793005 + 11634580027462260723) & ((1 << 64) - 1)
        xs = (((state >> 18) ^ state) >> 27) & M32
        rot = state >> 59
        key.append(((xs >> rot) | (xs << ((32 - rot) & 31))) & M32)
    return key


class StdRng:
    def __init__(self, key, word_pos=0):
        self.key = list(key)
        self.word_pos = word_pos
        self._blk, self._buf = None, None
        self.fr_rejections = []      # word_pos of every rejected Fr candidate
        self.fr_accepts = []         # ... and of every accepted one
        self.range_rejections = []   # word_pos of every rejected gen_range trial

    @classmethod
    def seed_from_u64(cls, seed):
        return cls(key_from_u64(seed))

    @classmethod
    def from_state(cls, b):
        w = struct.unpack("<8IQ", bytes(b))
        return cls(w[:8], w[8])

    def state(self):
        return struct.pack("<8IQ", *self.key, self.word_pos)

    def clone(self):
        return StdRng(self.key, self.word_pos)

    def word(self, pos):
        blk = pos >> 4
        if blk != self._blk:
            self._blk, self._buf = blk, chacha12_block(self.key, blk)
        return self._buf[pos & 15]

    def next_u32(self):
        v = self.word(self.word_pos)
        self.word_pos += 1
        return v

    def next_u64(self):
        lo = self.next_u32()
        return lo | (self.next_u32() << 32)

    def fr_int(self):
        """Fr::rand: the accepted 255-bit value (the limbs are the Montgomery form: the value IS what goes over the wire)"""
        while True:
            at = self.word_pos
            v = 0
            for i in range(4):
                v |= self.next_u64() << (64 * i)
            v &= (1 << 255) - 1
            if v < R:
                self.fr_accepts.append(at)
                return v
            self.fr_rejections.append(at)

    def fr(self, n=1):
        return b"".join(self.fr_int().to_bytes(32, "little") for _ in range(n))

    def gen_range(self, rng_):
        zone = (((rng_ << (32 - rng_.bit_length())) & M32) - 1) & M32
        while True:
            at = self.word_pos
            m = self.next_u32() * rng_
            if (m & M32) <= zone:
                return m >> 32
            self.range_rejections.append(at)

    def shuffle(self, n):
        p = list(range(n))
        for i in range(n - 1, 0, -1):
            j = self.gen_range(i + 1)
            p[i], p[j] = p[j], p[i]
        return p

    def split(self):
        """ChaCha12Rng::from_rng(&mut self)"""
        return StdRng([self.next_u32() for _ in range(8)], 0)

    def shuffle_draws(self, ell):
        """the draws of one generate_whisk_shuffle_proof (whisk.rs:144-179): (perm, k, blinders, rand, state after k)"""
        perm = self.shuffle(ell)
        k = self.fr(1)
        mid = self.state()
        mb = self.fr(4)
        return perm, k, mb, self.fr(3 * (ell + 4) + 9), mid
