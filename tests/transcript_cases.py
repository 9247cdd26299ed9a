"""Case sets, file format and comparison for tests/device/transcript_check.hip (TEST INFRASTRUCTURE ONLY).

A case is a start state (27 words: 25 state words, pos, pos_begin), a list of operations and a message offset.  Every set is
deterministic (seeded random.Random) and every expectation comes from tests/strobe_ref.py: reference(case) gives the final 27
words, every challenge (Montgomery form) with its attempt count, and the reference's trace.

Start states: STROBE holds pos_begin = 0 (after a permutation) or the position after an operation's first header byte, which
lies below pos once the second header byte is written.  The sweep takes pos_begin from {0, 1, pos - 1, pos, 166} and keeps what is
reachable between operations, pos_begin = 0 or pos_begin < pos; pos_begin = pos and 166 occur only inside begin_op and are left out
when generating (the program itself accepts any pos <= 165, pos_begin <= 166).
"""
import functools
import os
import random
import struct

from tests import check_harness as ch
from tests import strobe_ref as sr
from tests.check_harness import list_operations   # noqa: F401

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(_ROOT, "tests", "device", "transcript_check.hip")
CSRC = os.path.join(_ROOT, "curdleproofs_amd", "csrc")

HELPERS = {"bits_unshuffle32": (1, 1), "bits_shuffle32": (1, 1), "bits_split64": (2, 2), "bits_join64": (2, 2)}
HOST_TABLE = dict({"strobe_host": (0, 0)}, **HELPERS)
DEVICE_ENGINES = ("wave", "wave_lds", "lane", "strobe_dev")
DEVICE_TABLE = dict({e: (0, 0) for e in DEVICE_ENGINES}, **HOST_TABLE)
SETS = ("permutation", "sweep", "streams", "retries")

CODES = {"init": 1, "meta_ad": 2, "append_message": 3, "append_begin": 4, "absorb": 5, "append_scalar": 6, "challenge_scalar": 7, "keccak": 8,
         "round_trip": 9}

# the product's labels (grep '"[a-z_0-9]*"' over curdleproofs_amd/csrc): 7 ("dom-sep") to 31 bytes
LONGEST_LABEL = b"tracker_opening_proof_challenge"
assert len(LONGEST_LABEL) == 31
LABEL63 = b"a_label_of_sixty_three_bytes_which_no_caller_uses_but_strobe_ok"      # 64 + 2 + 63 + 4 + 2 = 135: the scalar of a challenge
assert len(LABEL63) == 63                                                           # appended back under it crosses the boundary


class Case:
    def __init__(self, name, state, ops, msg_offset=0):
        self.name, self.state, self.ops, self.msg_offset = name, list(state), list(ops), msg_offset
        assert len(self.state) == 27

    @property
    def pos(self):
        return self.state[25]

    def prefix(self, k):
        return Case(self.name, self.state, self.ops[:k], self.msg_offset)


def random_state(rnd, pos=0, pos_begin=0):
    return [rnd.getrandbits(64) for _ in range(25)] + [pos, pos_begin]


# ---------------------------------------------------------------- the reference's answer
def oracle_permute(orc):
    """the oracle's permutation on 25 words (pinned against the Python permutation by tests/test_transcript_check_cpu.py): the
    STROBE layer of the reference stays Python, only the 24 rounds run in C"""
    def permute(words):
        return sr.bytes_to_state(orc.keccak_f1600(sr.state_to_bytes(words)))
    return permute


def reference(case, permute=sr.keccak_f1600):
    """(final 27 words, [(scalar in Montgomery form, attempts)], trace)"""
    t = sr.Transcript.from_words(case.state, permute)
    chal = []
    for op in case.ops:
        k = op[0]
        if k == "init":
            trace = t.trace
            t = sr.Transcript(op[1], permute)
            t.s.trace = trace + [("op", "init", 0)] + t.s.trace
        elif k == "meta_ad":
            t.meta_ad(op[1], op[2])
        elif k == "append_message":
            t.append_message(op[1], op[2])
        elif k == "append_begin":
            t.append_begin(op[1], op[2])
        elif k == "absorb":
            t.absorb(op[1])
        elif k == "append_scalar":
            t.append_scalar(op[1], op[2])
        elif k == "challenge_scalar":
            x, attempts = t.get_and_append_challenge(op[1])
            chal.append((sr.to_mont(x), attempts))
        elif k == "keccak":
            t.s.trace.append(("op", "keccak", t.s.pos))
            t.s._permute()
        elif k == "round_trip":
            t = sr.Transcript(strobe=_reload(t.s))
        else:
            raise ValueError(k)
    return t.to_words(), chal, t.trace


def _reload(s):
    n = sr.Strobe.from_words(s.to_words(), s.permute)
    n.trace = s.trace + [("op", "round_trip", s.pos)]
    return n


# ---------------------------------------------------------------- the case sets
def permutation_set():
    rnd = random.Random(0x6b656363)
    ones = (1 << 64) - 1
    cases = [Case("zero", [0] * 27, [("keccak",)]), Case("ones", [ones] * 25 + [0, 0], [("keccak",)])]

    def bit(i):
        return [(1 << (i % 64)) if w == i // 64 else 0 for w in range(25)]
    for i in range(1600):       # one per state bit: a wrong lane, half or rotation amount of the gather plan, in any round
        cases.append(Case("bit_%d" % i, bit(i) + [0, 0], [("keccak",)]))
    for i in (0, 63, 64, 959, 960, 1599):      # 960..1023 = word 15, the lane gap
        cases.append(Case("all_but_bit_%d" % i, [w ^ ones for w in bit(i)] + [0, 0], [("keccak",)]))
    for i in range(64):
        cases.append(Case("random_%d" % i, random_state(rnd), [("keccak",)]))
    for i in range(8):          # the empty lanes stay clear between calls
        cases.append(Case("random_3x_%d" % i, random_state(rnd), [("keccak",)] * 3))
    cases.append(Case("round_trip", random_state(rnd, 17, 5), [("round_trip",), ("keccak",), ("round_trip",)]))
    return cases


SWEEP_LABELS = (b"x", b"dom-sep", b"curdleproofs_step1", LONGEST_LABEL)      # 1, 7, 18, 31 bytes
SWEEP_DATA = (0, 1, 32, 48, sr.RATE - 2)
DISTINCT_BYTES = int.from_bytes(bytes(range(0x21, 0x41)), "little")          # a distinct value in every byte, below r (top byte 0x40)
SWEEP_SCALARS = (0, 1, sr.R_FR - 1, DISTINCT_BYTES)
assert DISTINCT_BYTES < sr.R_FR


def sweep_states():
    """(pos, pos_begin) for every pos with every reachable pos_begin of {0, 1, pos - 1, pos, 166}"""
    out = []
    for pos in range(sr.RATE):
        for pb in sorted({0, 1, pos - 1, pos, 166}):
            if pb == 0 or 0 < pb < pos:
                out.append((pos, pb))
    return out


def sweep_set():
    rnd = random.Random(0x73776565)
    cases = []
    for pos, pb in sweep_states():
        st = random_state(rnd, pos, pb)
        tag = "pos%d_begin%d" % (pos, pb)

        def add(name, ops):
            cases.append(Case("%s_%s" % (tag, name), st, ops, msg_offset=len(cases) % 8))
        for lb in SWEEP_LABELS:
            for n in SWEEP_DATA:
                add("append_message_%d_%d" % (len(lb), n), [("append_message", lb, rnd.randbytes(n))])
        for i, x in enumerate(SWEEP_SCALARS):
            add("append_scalar_%d" % i, [("append_scalar", SWEEP_LABELS[1 + i % 3], x)])
        add("challenge_11", [("challenge_scalar", b"gprod_alpha")])
        add("challenge_31", [("challenge_scalar", LONGEST_LABEL)])
        add("meta_ad_pair", [("meta_ad", rnd.randbytes(7), False), ("meta_ad", rnd.randbytes(4), True)])
        add("streamed", [("append_begin", SWEEP_LABELS[2], 8 + 48), ("absorb", (1).to_bytes(8, "little")), ("absorb", rnd.randbytes(48))])
    # targeted: a message longer than two full blocks that starts mid-block, and one of the longest the host test uses
    cases.append(Case("long_400_from_77", random_state(rnd, 77, 30), [("append_message", SWEEP_LABELS[2], rnd.randbytes(400))], 3))
    cases.append(Case("long_12104_from_131", random_state(rnd, 131, 0), [("append_message", SWEEP_LABELS[1], rnd.randbytes(12104))], 5))
    return cases


def step1_ops(rnd, ell):
    """the prefix k_transcript_step1 hashes: four Vec<G1Affine> of ell points, M, ell challenges"""
    ops = [("init", b"curdleproofs")]
    for _ in range(4):
        ops += [("append_begin", b"curdleproofs_step1", 8 + 48 * ell), ("absorb", ell.to_bytes(8, "little")), ("absorb", rnd.randbytes(48 * ell))]
    ops += [("append_begin", b"curdleproofs_step1", 48), ("absorb", rnd.randbytes(48))]
    return ops + [("challenge_scalar", b"curdleproofs_vec_a")] * ell


def streams_set():
    rnd = random.Random(0x73747265)
    shapes = []
    for ell in (1, 3, 4, 7):            # 48 ell + 8 = 56, 152, 200, 344 bytes: below, around and above one and two rate blocks
        shapes.append(("step1_ell%d" % ell, [0] * 27, step1_ops(rnd, ell)))
    shapes.append(("tracker", [0] * 27, [("init", b"whisk_opening_proof")] + [("append_message", b"tracker_opening_proof", rnd.randbytes(48)) for _ in range(6)] +
                   [("challenge_scalar", LONGEST_LABEL)]))
    loop = []
    for _ in range(12):
        loop += [("append_message", b"ipa_loop", rnd.randbytes(48)) for _ in range(4)] + [("challenge_scalar", b"ipa_gamma")]
    shapes.append(("ipa_loop_x12", random_state(rnd, 64, 0), loop))
    return [Case("%s_offset%d" % (name, off), st, ops, off) for name, st, ops in shapes for off in range(9)]


# Start states (random.Random(seed), pos = seed % 166, pos_begin = 0) whose next challenge under the label needs exactly one / exactly
# two retries: found by find_retry_seeds() below, which walks the seeds upwards and stops at the first hits;
# tests/test_transcript_check_cpu.py re-derives the attempt counts from the reference.
RETRY_LABEL = b"curdleproofs_vec_a"
RETRY1_SEEDS = (19, 43, 46, 52, 72, 75, 91, 106, 108, 116, 133, 138, 139, 144, 157, 173)
RETRY2_SEEDS = (4, 44)
RETRY1_SEEDS_LABEL63 = (17, 27)


def retry_state(seed):
    return random_state(random.Random(seed), seed % sr.RATE, 0)


def find_retry_seeds(permute, label, retries, count, limit=100000):
    out = []
    for seed in range(limit):
        _, chal, _ = reference(Case("", retry_state(seed), [("challenge_scalar", label)]), permute)
        if chal[0][1] == retries + 1:
            out.append(seed)
            if len(out) == count:
                break
    return tuple(out)


def retries_set():
    cases = []
    for seeds, label, tag in ((RETRY1_SEEDS, RETRY_LABEL, "one_retry"), (RETRY2_SEEDS, RETRY_LABEL, "two_retries"), (RETRY1_SEEDS_LABEL63, LABEL63, "one_retry_label63")):
        for s in seeds:      # the challenge, then a scalar and another challenge on the state it leaves
            cases.append(Case("%s_seed%d" % (tag, s), retry_state(s), [("challenge_scalar", label), ("append_scalar", b"gprod_step1", DISTINCT_BYTES),
                                                                      ("challenge_scalar", b"gprod_alpha")], s % 8))
    return cases


_BUILDERS = {"permutation": permutation_set, "sweep": sweep_set, "streams": streams_set, "retries": retries_set}
_cache = {}


def cases_of(name):
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


_expected = {}


def expected(name, orc):
    """the reference's answers for a set, computed once per process: [(words, challenges, trace)].  The permutation set runs the
    Python permutation; the other sets run the Python STROBE layer over the oracle's permutation."""
    if name not in _expected:
        permute = sr.keccak_f1600 if name == "permutation" else oracle_permute(orc)
        _expected[name] = [reference(c, permute) for c in cases_of(name)]
    return _expected[name]


def helper_words():
    rnd = random.Random(0x62697473)
    w32 = [0, 0xffffffff, 0x55555555, 0xaaaaaaaa] + [1 << i for i in range(32)] + [rnd.getrandbits(32) for _ in range(256)]
    w64 = [0, (1 << 64) - 1, 0x5555555555555555, 0xaaaaaaaaaaaaaaaa] + [1 << i for i in range(64)] + [rnd.getrandbits(64) for _ in range(256)]
    return w32, w64


def helper_records():
    w32, w64 = helper_words()
    pairs = [[v & 0xffffffff, v >> 32] for v in w64]
    return [("bits_unshuffle32", [[v] for v in w32]), ("bits_shuffle32", [[v] for v in w32]), ("bits_split64", pairs), ("bits_join64", pairs)]


# ---------------------------------------------------------------- the real transcripts' schedule (for the coverage count)
def proof_schedule(ell):
    """the operations of one Curdleproofs proof transcript for ell ciphertexts (n = ell + 4 = 2^L), as the verifier walks them
    (curdleproofs_amd/csrc/host_transcript.hpp): only lengths and labels matter for the positions, the data is zero"""
    n = ell + 4
    L = n.bit_length() - 1
    assert 1 << L == n
    pt, ops = bytes(48), [("init", b"curdleproofs")]

    def point(label, k=1):
        ops.extend([("append_message", label, pt)] * k)

    def vec(label, count, width):
        ops.extend([("append_begin", label, 8 + width * count), ("absorb", count.to_bytes(8, "little")), ("absorb", bytes(width * count))])

    def scalar(label):
        ops.append(("append_scalar", label, 1))

    def chal(label, k=1):
        ops.extend([("challenge_scalar", label)] * k)
    for _ in range(4):
        vec(b"curdleproofs_step1", ell, 48)
    point(b"curdleproofs_step1")
    chal(b"curdleproofs_vec_a", ell)
    point(b"same_perm_step1", 2)
    ops.append(("append_begin", b"same_perm_step1", 8 + 32 * ell))
    ops.append(("absorb", ell.to_bytes(8, "little")))
    ops.extend([("absorb", bytes(32))] * ell)
    chal(b"same_perm_alpha"), chal(b"same_perm_beta")
    point(b"gprod_step1"), scalar(b"gprod_step1"), chal(b"gprod_alpha")
    point(b"gprod_step2"), scalar(b"gprod_step2"), chal(b"gprod_beta")
    point(b"ipa_step1", 2), scalar(b"ipa_step1"), point(b"ipa_step1", 2), chal(b"ipa_alpha"), chal(b"ipa_beta")
    for _ in range(L):
        point(b"ipa_loop", 4), chal(b"ipa_gamma")
    point(b"sameexp_points", 10), chal(b"same_scalar_alpha")
    point(b"same_msm_step1", 3), vec(b"same_msm_step1", n, 48), vec(b"same_msm_step1", n, 48), point(b"same_msm_step1", 3), chal(b"same_msm_alpha")
    for _ in range(L):
        point(b"same_msm_loop", 6), chal(b"same_msm_gamma")
    return ops


# ---------------------------------------------------------------- the program: build, file format, run
build_host_twin = functools.partial(ch.build_host_twin, SRC, name="transcript_check_host")      # (out_dir, extra=())


def encode_case(case):
    blob, ops = bytearray(), []

    def put(b):
        o = len(blob)
        blob.extend(b)
        return o
    for op in case.ops:
        k = op[0]
        if k in ("init", "challenge_scalar"):
            ops.append((CODES[k], put(op[1]), len(op[1]), 0))
        elif k == "meta_ad":
            ops.append((CODES[k], put(op[1]), len(op[1]), int(op[2])))
        elif k == "append_message":
            ops.append((CODES[k], put(op[1] + op[2]), len(op[1]), len(op[2])))
        elif k == "append_begin":
            ops.append((CODES[k], put(op[1]), len(op[1]), op[2]))
        elif k == "absorb":
            ops.append((CODES[k], put(op[1]), len(op[1]), 0))
        elif k == "append_scalar":
            a = put(op[1])
            ops.append((CODES[k], a, len(op[1]), put(sr.to_mont(op[2]).to_bytes(32, "little"))))
        else:
            ops.append((CODES[k], 0, 0, 0))
    n = len(blob)
    blob.extend(bytes(-n % 8))
    return (struct.pack("<4I27Q", len(ops), n, case.msg_offset, 0, *case.state) + b"".join(struct.pack("<4I", *o) for o in ops) + bytes(blob))


def engine_record(engine, cases):
    return ch.pack_record(engine, 0, len(cases), b"".join(encode_case(c) for c in cases))


def run_engine(exe, engine, cases, work_dir, tag, timeout=120):
    """one process: every case through `engine`; [(27 words, [(scalar, attempts)])], one per case"""
    with open(ch.run_file(exe, engine_record(engine, cases), work_dir, tag, timeout, "1 records, %d rows" % len(cases)), "rb") as f:
        data = f.read()
    name, words, _, rows = struct.unpack_from(ch.HEADER, data, 0)
    assert name.rstrip(b"\0").decode() == engine and rows == len(cases)
    o, out = 64, []
    for c in cases:
        nchal, _ = struct.unpack_from("<II", data, o)
        assert nchal == sum(1 for op in c.ops if op[0] == "challenge_scalar"), c.name
        st = list(struct.unpack_from("<27Q", data, o + 8))
        o += 8 + 27 * 8
        chal = []
        for _ in range(nchal):
            v = struct.unpack_from("<5Q", data, o)
            chal.append((sum(x << (64 * i) for i, x in enumerate(v[:4])), v[4]))
            o += 40
        out.append((st, chal))
    assert o == len(data)
    return out


def run_rows(exe, records, work_dir, tag, timeout=120):
    return ch.run(exe, HELPERS, records, work_dir, tag, timeout)


# ---------------------------------------------------------------- comparison
WORD_NAMES = ["state word %d" % i for i in range(25)] + ["pos", "pos_begin"]


def first_difference(got, want):
    """None, or a description of the first differing word of (27 words, challenges)"""
    for i in range(27):
        if got[0][i] != want[0][i]:
            return "%s: got 0x%x, expected 0x%x" % (WORD_NAMES[i], got[0][i], want[0][i])
    if len(got[1]) != len(want[1]):
        return "%d challenges, expected %d" % (len(got[1]), len(want[1]))
    for j, (g, w) in enumerate(zip(got[1], want[1])):
        if g[0] != w[0]:
            return "challenge %d: got 0x%x, expected 0x%x" % (j, g[0], w[0])
        if g[1] != w[1]:
            return "challenge %d: %d attempts, expected %d" % (j, g[1], w[1])
    return None


def first_bad_operation(exe, engine, case, permute, work_dir):
    """the index of the first operation after which `engine` leaves the reference: the case's prefixes, one more process"""
    prefixes = [case.prefix(k) for k in range(1, len(case.ops) + 1)]
    got = run_engine(exe, engine, prefixes, work_dir, "prefixes_" + engine)
    for k, (p, g) in enumerate(zip(prefixes, got)):
        w, chal, _ = reference(p, permute)
        if first_difference(g, (w, chal)):
            return k
    return None


def assert_same(engine, cases, got, want, who="the reference", locate=None):
    """every case of `got` against `want` ([(words, challenges, ...)]), word for word; returns the number of cases compared.  A failure
    names the engine, the case, the start pos and the first differing word; locate(case) adds the operation index."""
    assert len(got) == len(want) == len(cases)
    n = 0
    for c, g, w in zip(cases, got, want):
        d = first_difference(g, w)
        if d:
            k = locate(c) if locate else None
            at = "" if k is None else ", operation %d (%s)" % (k, c.ops[k][0])
            raise AssertionError("engine %s, case %s (start pos %d, pos_begin %d, message offset %d)%s differs from %s: %s" % (
                engine, c.name, c.state[25], c.state[26], c.msg_offset, at, who, d))
        n += 1
    return n


def check_helpers(got):
    """the four bit helpers against Python bit loops; returns the number of rows checked"""
    w32, w64 = helper_words()
    by = dict(got)

    def unshuffle(v, bits):
        h = bits // 2
        return sum(((v >> (2 * i)) & 1) << i for i in range(h)) | sum(((v >> (2 * i + 1)) & 1) << (h + i) for i in range(h))
    n = 0
    for i, v in enumerate(w32):
        u = int(by["bits_unshuffle32"][i, 0])
        assert u == unshuffle(v, 32), "bits_unshuffle32(0x%x) = 0x%x" % (v, u)
        s = int(by["bits_shuffle32"][i, 0])
        assert unshuffle(s, 32) == v, "bits_shuffle32(0x%x) = 0x%x" % (v, s)
        n += 2
    for i, v in enumerate(w64):
        e, o = int(by["bits_split64"][i, 0]), int(by["bits_split64"][i, 1])
        assert e | (o << 32) == unshuffle(v, 64), "bits_split64(0x%x) = (0x%x, 0x%x)" % (v, e, o)
        j = int(by["bits_join64"][i, 0]) | (int(by["bits_join64"][i, 1]) << 32)       # read v as (even, odd)
        assert unshuffle(j, 64) == v, "bits_join64(0x%x, 0x%x) = 0x%x" % (v & 0xffffffff, v >> 32, j)
        n += 2
    return n


def check_helper_round_trips(exe, records, got, work_dir):
    """split o join, join o split, shuffle o unshuffle and unshuffle o shuffle are the identity: each helper on the other's output"""
    by, inp = dict(got), dict(records)
    again = [("bits_shuffle32", by["bits_unshuffle32"].tolist()), ("bits_unshuffle32", by["bits_shuffle32"].tolist()),
             ("bits_join64", by["bits_split64"].tolist()), ("bits_split64", by["bits_join64"].tolist())]
    back = run_rows(exe, again, work_dir, "helpers_back")
    for (name, a), src in zip(back, ("bits_unshuffle32", "bits_shuffle32", "bits_split64", "bits_join64")):
        assert a.tolist() == inp[src], "%s after %s is not the identity" % (name, src)
