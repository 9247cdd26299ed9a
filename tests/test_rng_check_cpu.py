"""The draws of the reference's provers without a GPU: the Python model of StdRng and its samplers (tests/stdrng_ref.py) against the oracle's
(oracle/stdrng.h, which the reference's two known-answer tests pin), what the case set of tests/rng_cases.py covers, the host twin of
tests/device/rng_check.hip — curdleproofs_amd/csrc/rng.hpp compiled by g++ as plain C++ — row by row against the model, once more under the
undefined-behaviour and address sanitizers as a stand-alone program, the two host-only entry points of the C-ABI, and the names."""
import ctypes
import os
import re
import struct

import pytest

from tests import rng_cases as rc
from tests import stdrng_ref as sr
from tests.stdrng_ref import StdRng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cpx_rng_from_u64", "cpx_rng_split", "cpx_rng_fr", "cpx_rng_shuffle_draws", "cpx_whisk_generate_shuffle_proofs_rng", "cpx_batch_prove_rng")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return rc.build_host_twin(tmp_path_factory.mktemp("rng_check"))


@pytest.mark.parametrize("seed", [0, 1, 7, (1 << 64) - 1])
def test_model_against_the_oracle(orc, seed):
    """key, the first 3000 words, then Fr::rand, a shuffle, Fr::rand again from wherever that left the stream"""
    o, m = orc.rng(seed), StdRng.seed_from_u64(seed)
    assert o.key() == struct.pack("<8I", *m.key)
    assert [o.u32() for _ in range(3000)] == [m.next_u32() for _ in range(3000)]
    for n in (1, 5, 124, 2):
        assert o.fr(40) == m.fr(40)
        assert o.shuffle(n) == m.shuffle(n)
        o.u32(), m.next_u32()               # (an odd offset for the next round)
    assert o.fr(300) == m.fr(300) and o.u32() == m.next_u32()
    assert m.fr_rejections and m.range_rejections


def test_model_seeks():
    """word_pos is the whole position: a stream restarted from its state, anywhere, goes on with the same words"""
    a = StdRng.seed_from_u64(5)
    ws = [a.next_u32() for _ in range(100)]
    for pos in (0, 1, 15, 16, 17, 63, 99):
        assert StdRng(a.key, pos).next_u32() == ws[pos]
    b = StdRng.from_state(StdRng(a.key, 37).state())
    assert b.next_u64() == ws[37] | (ws[38] << 32) and b.word_pos == 39
    c = StdRng(a.key, 15)
    assert c.next_u64() == ws[15] | (ws[16] << 32)      # across the block boundary
    child = StdRng(a.key, 8).split()
    assert child.key == ws[8:16] and child.word_pos == 0


def test_fr_case_set_coverage():
    """what cpx_rng_fr is run on (tests/test_gpu_rng.py): every property the kernel's window walk can get wrong has a stream that shows it"""
    cases = rc.fr_cases()
    assert {n for n, _ in cases} >= set(rc.N_EACH) and all(len(st) == 65 == len(set(st)) for _, st in cases)
    starts = {StdRng.from_state(s).word_pos % 16 for s in rc.pool()}
    assert starts == set(range(16))
    assert any(StdRng.from_state(s).word_pos == (1 << 36) - 40 for s in rc.pool())
    rej_straddle = acc_straddle = run3 = last63 = first64 = False
    for n, states in cases:
        for s in states:
            c = rc.candidates(StdRng.from_state(s), n)
            start = c[0][0]
            assert all(p == start + 8 * i for i, (p, _) in enumerate(c)) and c[-1][1] and sum(a for _, a in c) == n
            for p, a in c:
                if p % 16 > 8:                       # eight words from an offset above 8 cross into the next block
                    acc_straddle |= a
                    rej_straddle |= not a
            acc = [a for _, a in c]
            run3 |= any(not any(acc[i:i + 3]) for i in range(len(acc) - 2))
            last63 |= len(c) % rc.WINDOW == 0        # the last draw is the last candidate of a window
            first64 |= len(c) % rc.WINDOW == 1 and len(c) > 1
    assert rej_straddle and acc_straddle and run3 and last63 and first64
    # the high start: the counter's high word changes inside the first draws
    hi = StdRng.from_state(rc.pool()[16])
    assert hi.word_pos >> 36 == 0 and rc.candidates(hi, 63)[-1][0] >> 36 == 1
    # the two searched cases are what they are meant to be
    (s_last, n_last), (s_first, n_first), _ = rc.edge_cases()
    assert len(rc.candidates(StdRng.from_state(s_last), n_last)) == 64 and len(rc.candidates(StdRng.from_state(s_first), n_first)) == 65


@pytest.mark.parametrize("ell", rc.SHUFFLE_ELLS)
def test_shuffle_case_set_coverage(ell):
    """cpx_rng_shuffle_draws: gen_range rejections, a run of three, Fr phases that start at odd offsets behind the shuffle"""
    runs, offs = 0, set()
    for s in rc.shuffle_states(ell):
        rng = StdRng.from_state(s)
        perm = rng.shuffle(ell)
        assert sorted(perm) == list(range(ell))
        offs.add(rng.word_pos % 16)
        rj = rng.range_rejections
        assert rj
        runs = max([runs] + [1 + max(k for k in range(len(rj) - i) if rj[i + k] == rj[i] + k) for i in range(len(rj))])
    assert runs >= 3 and len(offs) >= 2
    want = rc.shuffle_expected(ell, rc.shuffle_states(ell))
    assert all(len(w[3]) == 32 * (3 * (ell + 4) + 9) and w[4] != w[5] for w in want)


def test_seed_zero_is_the_reference_kat_stream(orc):
    """whisk.rs:416-456 from the number 0: 248 draws make the trackers, then the model's shuffle draws are the oracle's, in the oracle's order"""
    o, m = orc.rng(0), StdRng.seed_from_u64(0)
    assert o.fr(248) == m.fr(248)
    perm, k, mb, rand, _ = m.shuffle_draws(124)
    assert (o.shuffle(124), o.fr(1), o.fr(4), o.fr(3 * 128 + 9)) == (perm, k, mb, rand)
    assert o.fr(8) == m.fr(8)


def test_twin_against_the_model(twin, tmp_path):
    assert rc.list_operations(twin) == rc.TABLE
    records = rc.check_records()
    got = rc.run_check(twin, records, tmp_path, "all")
    assert rc.assert_rows(records, got, rc.check_expected(), ("host twin", "model")) == sum(len(r) for _, r in records) > 1500


def test_twin_under_sanitizers(tmp_path):
    """the twin built with -fsanitize=undefined,address (no recovery) as a stand-alone program: the rotates, the shift by clz and the PCG
    rotation by 32 - rot are what this run is for"""
    exe = rc.build_host_twin(tmp_path, extra=["-O1", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"], name="rng_check_san")
    records = rc.check_records()
    got = rc.run_check(exe, records, tmp_path, "san")
    assert rc.assert_rows(records, got, rc.check_expected(), ("sanitized twin", "model")) == sum(len(r) for _, r in records)


def test_the_check_notices_a_wrong_word(twin, tmp_path):
    records = rc.check_records()[:2]
    got = rc.run_check(twin, records, tmp_path, "two")
    bad = [(n, a.copy()) for n, a in got]
    bad[1][1][3, 5] ^= 1
    with pytest.raises(AssertionError, match="next_u32 row 3"):
        rc.assert_rows(records, bad, rc.check_expected()[:2], ("host twin", "model"))


@pytest.fixture(scope="module")
def lib():
    from curdleproofs_amd.build import build
    build()
    import curdleproofs_amd as cpx
    return cpx.load_library()


def test_host_only_entry_points(lib):
    """cpx_rng_from_u64 and cpx_rng_split need no context and no GPU"""
    import curdleproofs_amd as cpx
    st = (ctypes.c_uint8 * 40)()
    for seed in rc.SEEDS:
        assert lib.cpx_rng_from_u64(seed, st) == cpx.CPX_OK and bytes(st) == StdRng.seed_from_u64(seed).state()
    assert lib.cpx_rng_from_u64(0, None) == cpx.CPX_ERR_ARG
    for start in (0, 3, 13, rc.HIGH_POS):
        m = StdRng(sr.key_from_u64(9), start)
        parent = (ctypes.c_uint8 * 40).from_buffer_copy(m.state())
        out = (ctypes.c_uint8 * (40 * 5))()
        assert lib.cpx_rng_split(parent, 5, out) == cpx.CPX_OK
        assert bytes(out) == b"".join(m.split().state() for _ in range(5)) and bytes(parent) == m.state()
        assert m.word_pos == start + 40
    # count = 0: a no-op; NULL with work to do and a position too close to 2^64: CPX_ERR_ARG, nothing written
    before = bytes(parent)
    assert lib.cpx_rng_split(parent, 0, None) == cpx.CPX_OK and lib.cpx_rng_split(None, 0, None) == cpx.CPX_OK
    assert lib.cpx_rng_split(parent, 2, None) == cpx.CPX_ERR_ARG and lib.cpx_rng_split(None, 2, out) == cpx.CPX_ERR_ARG
    late = (ctypes.c_uint8 * 40).from_buffer_copy(StdRng(m.key, sr.POS_LIMIT).state())
    filled = bytes(out)
    assert lib.cpx_rng_split(late, 1, out) == cpx.CPX_ERR_ARG and bytes(out) == filled and bytes(parent) == before
    assert bytes(late) == StdRng(m.key, sr.POS_LIMIT).state()
    # the context calls refuse NULL before anything else
    assert lib.cpx_rng_fr(None, 1, None, 1, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_rng_shuffle_draws(None, 1, None, None, None, None, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_generate_shuffle_proofs_rng(None, 1, None, None, None, None, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_batch_prove_rng(None, None, None, None, None, None) == cpx.CPX_ERR_ARG


def test_names_everywhere(lib):
    import curdleproofs_amd as cpx
    hdr = open(os.path.join(ROOT, "include", "cpx.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "whisk_mi355x.rs")).read()
    for name in NAMES:
        assert name in cpx.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, hdr), "include/cpx.h lacks %s" % name
        assert re.search(r"pub fn %s\(" % name, ffi), "integration/rust/ffi.rs lacks %s" % name
    for name in ("cpx_rng_fr", "cpx_whisk_generate_shuffle_proofs_rng"):
        assert name + "(" in rs, "integration/rust/whisk_mi355x.rs does not call %s" % name
    assert "k_rng_draw" in cpx.Context.KERNELS and '"k_rng_draw"' in hdr
    assert "cpx_rng_split" in hdr.split("SECRECY AND REUSE")[1].split("*/")[0]      # the warning names the way out
    from curdleproofs_amd import build
    assert "rng.hip" in build.SOURCES
    from curdleproofs_amd.rng import StdRng as ProductRng
    assert ProductRng.seed_from_u64(0).state == StdRng.seed_from_u64(0).state()
