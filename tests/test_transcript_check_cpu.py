"""The reference of the transcripts (tests/strobe_ref.py: Keccak-f[1600], STROBE-128 and Merlin in plain Python), pinned against the
oracle; the case sets of tests/transcript_cases.py with the coverage they promise, asserted on the reference's trace alone; and the
host twin of tests/device/transcript_check.hip (cpx::Strobe and the bit helpers through g++) on every set, word for word against the
reference: state, pos, pos_begin, challenges and attempt counts.  This pins the harness that tests/test_gpu_transcript.py runs on
the device (file format, table, case counts) without a GPU.

The permutation set and the pinning run the Python permutation; for the other sets the reference's STROBE layer (Python) calls the
oracle's permutation, which the first test ties to the Python one on the whole permutation set."""
import random
import struct
import subprocess

import pytest

from tests import strobe_ref as sr
from tests import transcript_cases as tc


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return tc.build_host_twin(tmp_path_factory.mktemp("transcript_check"))


# ---------------------------------------------------------------- the reference against the oracle
def test_reference_permutation_equals_the_oracle(orc):
    cases = tc.cases_of("permutation")
    for c, (words, _, _) in zip(cases, tc.expected("permutation", orc)):        # (computed by the Python permutation)
        st = sr.state_to_bytes(c.state[:25])
        for _ in range(sum(1 for op in c.ops if op[0] == "keccak")):
            st = orc.keccak_f1600(st)
        assert sr.state_to_bytes(words[:25]) == st, c.name


def test_reference_merlin_equals_the_oracle(orc):
    t = sr.Transcript(b"test protocol")
    t.append_message(b"some label", b"some data")
    assert t.challenge_bytes(b"challenge", 32) == orc.merlin_test_vector()
    rnd = random.Random(7)
    for n in (0, 1, 47, 165, 166, 167, 400, 12104):
        msg = rnd.randbytes(n)
        t = sr.Transcript(b"curdleproofs", permute=sr.keccak_f1600 if n < 1000 else tc.oracle_permute(orc))
        t.append_message(b"lbl", msg)
        a, b = t.get_and_append_challenge(b"ch")[0], t.get_and_append_challenge(b"ch")[0]
        assert sr.to_mont(a).to_bytes(32, "little") + sr.to_mont(b).to_bytes(32, "little") == orc.challenges(msg), n


def test_reference_state_round_trip():
    rnd = random.Random(3)
    w = tc.random_state(rnd, 99, 42)
    assert sr.Strobe.from_words(w).to_words() == w


# ---------------------------------------------------------------- what the sets reach, from the reference's trace
def _trace(name, orc):
    return [e for _, _, tr in tc.expected(name, orc) for e in tr]


def test_sweep_reaches_every_position_and_every_split(orc):
    trace = _trace("sweep", orc)
    at = sr.op_positions(trace)
    every = set(range(sr.RATE))
    for op in ("append_message", "append_scalar", "challenge_scalar", "meta_ad", "meta_ad_more", "append_begin", "absorb"):
        assert {p for o, p in at if o == op} == every, op
    assert {k for k, n in sr.splits(trace, "scalar")} == set(range(1, 32))          # the 32 bytes cut at every interior point
    assert {k for k, n in sr.splits(trace, "len") if n == 4} == {1, 2, 3}             # the LE32 tail split 1/3, 2/2, 3/1
    headers = {e[1] for e in trace if e[0] == "header"}
    assert headers == every and 165 in headers                                        # 165: the two header bytes straddle the boundary
    ends = set(sr.ends(trace, "data"))
    assert 166 in ends and 165 in ends                                                # a message ending on the boundary, and one byte before
    assert any(e[0] == "bytes" and e[1] == "data" and e[3] > 2 * sr.RATE and e[2] % sr.RATE not in (0,) for e in trace)   # > two blocks, from mid-block
    # the sweep's own shape: every label and data length from every start state
    cases = tc.cases_of("sweep")
    assert {(c.state[25], c.state[26]) for c in cases} >= set(tc.sweep_states())
    assert {len(l) for l in tc.SWEEP_LABELS} == {1, 7, 18, 31} and set(tc.SWEEP_DATA) == {0, 1, 32, 48, 164}
    assert all(pb == 0 or pb < pos for pos, pb in tc.sweep_states()) and {pos for pos, _ in tc.sweep_states()} == every


def test_longest_label_is_the_products_longest():
    import os
    import re
    longest = 0
    for f in os.listdir(tc.CSRC):
        with open(os.path.join(tc.CSRC, f), errors="replace") as fh:
            for m in re.finditer(r'(?:append\w*|challenge\w*|Transcript \w+)\(\s*"([^"]+)"', fh.read()):
                longest = max(longest, len(m.group(1)))
    assert longest == len(tc.LONGEST_LABEL) == 31


def test_retry_cases_retry(orc):
    cases, exp = tc.cases_of("retries"), tc.expected("retries", orc)
    first = [chal[0][1] for _, chal, _ in exp]
    assert sum(1 for a in first if a == 2) >= 16 and sum(1 for a in first if a == 3) >= 2
    for c, a in zip(cases, first):
        assert a == (3 if "two_retries" in c.name else 2), c.name
    # the seeds are the first hits of the search, and the search is the reference's
    pm = tc.oracle_permute(orc)
    assert tc.find_retry_seeds(pm, tc.RETRY_LABEL, 1, len(tc.RETRY1_SEEDS)) == tc.RETRY1_SEEDS
    assert tc.find_retry_seeds(pm, tc.RETRY_LABEL, 2, len(tc.RETRY2_SEEDS)) == tc.RETRY2_SEEDS
    assert tc.find_retry_seeds(pm, tc.LABEL63, 1, len(tc.RETRY1_SEEDS_LABEL63)) == tc.RETRY1_SEEDS_LABEL63
    # a failed attempt followed by a scalar append that crosses the boundary (the 63-byte label)
    crossing = []
    for c, (_, _, tr) in zip(cases, exp):
        first = tr[:[e[:2] for e in tr].index(("op", "append_scalar"))]      # the first challenge alone
        if ("attempt", False) in first and sr.splits(first[first.index(("attempt", False)):], "scalar"):
            crossing.append(c.name)
    assert crossing == ["one_retry_label63_seed%d" % s for s in tc.RETRY1_SEEDS_LABEL63]


def test_streams_cross_blocks_at_every_offset(orc):
    cases = tc.cases_of("streams")
    assert {c.msg_offset for c in cases} == set(range(9))
    names = {c.name.rsplit("_offset", 1)[0] for c in cases}
    assert names == {"step1_ell1", "step1_ell3", "step1_ell4", "step1_ell7", "tracker", "ipa_loop_x12"}
    longest = {c.name: max(len(op[1]) for op in c.ops if op[0] == "absorb") for c in cases if c.name.startswith("step1")}
    assert {longest["step1_ell%d_offset0" % e] for e in (1, 3, 4, 7)} == {48, 144, 192, 336}     # below, around, above one block; above two


def test_positions_a_real_proof_visits(orc):
    """the (operation, pos) pairs of a whole proof transcript at ell = 28 and ell = 252 (positions depend on labels and lengths only)
    next to what the new sets visit: the figures of the pull request's description"""
    pm = tc.oracle_permute(orc)
    real = {}
    for ell in (28, 252):
        _, _, tr = tc.reference(tc.Case("proof", [0] * 27, tc.proof_schedule(ell)), pm)
        real[ell] = sr.op_positions(tr)
    sets = set()
    for name in tc.SETS:
        sets |= sr.op_positions(_trace(name, orc))
    ops = ("append_message", "append_begin", "absorb", "append_scalar", "challenge_scalar")
    count = {ell: len({(o, p) for o, p in real[ell] if o in ops}) for ell in real}
    new = len({(o, p) for o, p in sets if o in ops})
    print("(operation, pos) pairs: ell=28 proof %d, ell=252 proof %d, both %d, the case sets %d of %d" % (
        count[28], count[252], len({(o, p) for o, p in real[28] | real[252] if o in ops}), new, len(ops) * sr.RATE))
    assert new == len(ops) * sr.RATE
    assert all((o, p) in sets for ell in real for o, p in real[ell] if o in ops)      # whatever a proof visits, the sets visit


# ---------------------------------------------------------------- the host twin
def test_operation_table(twin):
    assert tc.list_operations(twin) == tc.HOST_TABLE


@pytest.mark.parametrize("name", tc.SETS)
def test_host_twin_equals_the_reference(twin, orc, tmp_path, name):
    cases, want = tc.cases_of(name), tc.expected(name, orc)
    assert cases
    got = tc.run_engine(twin, "strobe_host", cases, tmp_path, name, timeout=600)
    permute = sr.keccak_f1600 if name == "permutation" else tc.oracle_permute(orc)
    assert tc.assert_same("strobe_host", cases, got, want,
                          locate=lambda c: tc.first_bad_operation(twin, "strobe_host", c, permute, tmp_path)) == len(cases)


def test_bit_helpers(twin, tmp_path):
    records = tc.helper_records()
    got = tc.run_rows(twin, records, tmp_path, "helpers")
    assert tc.check_helpers(got) == 2 * sum(len(r) for _, r in records[::2])
    tc.check_helper_round_trips(twin, records, got, tmp_path)


def test_the_comparison_notices_a_wrong_word(twin, orc, tmp_path):
    """not vacuous: one flipped bit in a state word, a challenge or an attempt count fails, naming engine, case, start pos, operation"""
    cases, want = tc.cases_of("retries")[:3], tc.expected("retries", orc)[:3]
    got = tc.run_engine(twin, "strobe_host", cases, tmp_path, "ok")
    assert tc.assert_same("strobe_host", cases, got, want) == 3
    bad = [(list(st), list(ch)) for st, ch in got]
    bad[1][0][7] ^= 1 << 40
    with pytest.raises(AssertionError, match=r"engine strobe_host, case %s \(start pos %d, .*operation 2 \(challenge_scalar\).*state word 7" % (cases[1].name, cases[1].pos)):
        tc.assert_same("strobe_host", cases, bad, want, locate=lambda c: 2)
    bad = [(list(st), list(ch)) for st, ch in got]
    bad[2][1][0] = (bad[2][1][0][0], bad[2][1][0][1] + 1)
    with pytest.raises(AssertionError, match=r"challenge 0: 3 attempts, expected 2"):
        tc.assert_same("strobe_host", cases, bad, want)
    # and the operation index is found from the program itself: a case whose expectation is wrong from its second operation on
    c = cases[0]
    assert tc.first_bad_operation(twin, "strobe_host", c, tc.oracle_permute(orc), tmp_path) is None
    lie = tc.Case(c.name, c.state, [c.ops[0], ("append_scalar", b"gprod_step1", 5), c.ops[2]], c.msg_offset)
    ran = tc.run_engine(twin, "strobe_host", [c.prefix(k) for k in (1, 2, 3)], tmp_path, "lie")
    refs = [tc.reference(lie.prefix(k), tc.oracle_permute(orc)) for k in (1, 2, 3)]
    assert [tc.first_difference(g, w[:2]) is None for g, w in zip(ran, refs)] == [True, False, False]


def test_bad_records_are_refused(twin, tmp_path):
    """an unknown engine, offsets outside the blob, a position outside the rate, a label with a NUL byte, truncated or trailing bytes:
    a non-zero exit code before anything runs"""
    ok = tc.Case("ok", [0] * 27, [("append_message", b"label", b"data")])
    good = tc.engine_record("strobe_host", [ok])

    def patched(offset, fmt, value):
        b = bytearray(good)
        struct.pack_into(fmt, b, offset, value)
        return bytes(b)
    case0, ops0 = 64, 64 + 16 + 27 * 8
    blobs = {"unknown": tc.engine_record("wave_of_nothing", [ok]),
             "device_engine_on_host": tc.engine_record("wave", [ok]),
             "words": patched(48, "<I", 3),
             "pos": patched(case0 + 16 + 25 * 8, "<Q", 166),
             "pos_begin": patched(case0 + 16 + 26 * 8, "<Q", 167),
             "label_outside": patched(ops0 + 4, "<I", 1000),
             "data_outside": patched(ops0 + 12, "<I", 5),
             "opcode": patched(ops0, "<I", 10),
             "nul_label": tc.engine_record("strobe_host", [tc.Case("nul", [0] * 27, [("append_message", b"la\0el", b"data")])]),
             "msg_offset": patched(case0 + 8, "<I", 16),
             "short": good[:-8],
             "tail": good + b"\0\0\0"}
    for tag, blob in blobs.items():
        inp = tmp_path / (tag + ".in")
        inp.write_bytes(blob)
        r = subprocess.run([twin, str(inp), str(tmp_path / (tag + ".out"))], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "transcript_check:" in r.stderr, tag
    assert tc.run_engine(twin, "strobe_host", [ok], tmp_path, "good")
