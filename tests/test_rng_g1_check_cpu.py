"""G1Projective::rand without a GPU: the Python model (tests/stdrng_g1_ref.py) against the oracle's (oracle/stdrng.h, which the reference's
known-answer tests pin), what the case set of tests/rng_g1_cases.py covers, the host twin of tests/device/rng_g1_check.hip —
rng_fp_accept / rng_g1_candidate of rng.hpp and g1_28_point_from_x / g1_28_clear_cofactor of g1_28.hpp compiled by g++ as plain C++ — row
by row against the model, once more under the undefined-behaviour and address sanitizers as a stand-alone program, and the names."""
import os
import re

import pytest

from tests import rng_cases as rc
from tests import rng_g1_cases as gc
from tests import stdrng_g1_ref as g1
from tests.stdrng_ref import StdRng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cpx_rng_g1", "cpx_rng_instance_draws", "cpx_crs_generate", "cpx_g1_clear_cofactor")
KERNELS = ("k_rng_g1_scan", "k_rng_g1_sqrt", "k_rng_g1_select", "k_clear_cofactor")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return gc.build_host_twin(tmp_path_factory.mktemp("rng_g1_check"))


@pytest.mark.parametrize("seed", gc.SEEDS)
def test_model_against_the_oracle(orc, seed):
    """points, then a word, scalars and points again from wherever that left the stream: the points and the next word agree"""
    o, m = orc.rng(seed), StdRng.seed_from_u64(seed)
    w = g1.Walk(m)
    assert o.g1_affine(40) == w.g1_affine(40)
    assert o.u32() == m.next_u32()
    assert o.fr(3) == m.fr(3)
    assert o.g1_affine(5) == w.g1_affine(5)
    assert o.u32() == m.next_u32()
    kinds = {k for _, k, _ in w.tokens}
    assert kinds == {g1.REJECTED, g1.NO_ROOT, g1.POINT}


def test_generate_crs_is_the_model_from_seed_zero(orc):
    assert orc.generate_crs_points(28) == g1.g1_affine(StdRng.seed_from_u64(0), 35)


def test_case_set_coverage():
    """what cpx_rng_g1 is run on (tests/test_gpu_rng_g1.py): every property the scan's window walk and the selection can get wrong has a
    stream that shows it"""
    pool = gc.pool()
    assert {gc.rng_of(d).word_pos % 16 for d in pool} == set(range(16))
    assert {(c, n) for c, n in gc.SHAPES} == {(1, 1), (1, 300), (3, 65), (65, 1), (65, 8)}
    assert gc.model_points_needed() <= 200
    acc_cross = rej_cross = False
    for streams, n, _ in gc.g1_cases():
        for d in streams:
            tokens, pos = gc.walk(d, n)
            assert tokens[0][0] == gc.rng_of(d).word_pos and tokens[-1][2] == pos and tokens[-1][1] == g1.POINT
            assert all(a[2] == b[0] for a, b in zip(tokens, tokens[1:])) and sum(k == g1.POINT for _, k, _ in tokens) == n
            for at, kind, _ in tokens:
                if at % 16 > 4:                     # twelve words from an offset above 4 cross into the next block
                    rej_cross |= kind == g1.REJECTED
                    acc_cross |= kind != g1.REJECTED
    assert acc_cross and rej_cross
    # the high start: the counter's high word changes inside the first draws
    hi = pool[64]
    assert gc.rng_of(hi).word_pos >> 36 == 0 and gc.walk(hi, 8)[1] >> 36 == 1
    # the searched cases are what they are meant to be
    s = gc.searched()
    for name, at_index in (("last", gc.EDGE_CAP - 1), ("first", gc.EDGE_CAP)):
        d, need, rcap = s[name]
        accepted = [k for _, k, _ in gc.walk(d, need)[0] if k != g1.REJECTED]
        assert (need, rcap) == (gc.EDGE_NEED, gc.EDGE_CAP) and len(accepted) == at_index + 1 and gc.cap(need, rcap) == gc.EDGE_CAP
    for name in ("bool first", "straddle"):
        d, need, rcap = s[name]
        used = {at for at, _, _ in gc.walk(d, need)[0]}
        assert rcap == 0 and any(at in used for at in gc._edge_tokens(d, need)[name])
    d, need, _ = s["rejected2"]
    kinds = [k for _, k, _ in gc.walk(d, need)[0]]
    assert any(kinds[i] == kinds[i + 1] == g1.REJECTED for i in range(len(kinds) - 1))
    d, need, _ = s["noroot4"]
    acc = [k for _, k, _ in gc.walk(d, need)[0] if k != g1.REJECTED]
    assert any(all(k == g1.NO_ROOT for k in acc[i:i + 4]) for i in range(len(acc) - 3))
    # the default cap of a round, as rng_g1_plan.hpp states it
    assert [gc.default_cap(n) for n in (1, 2, 4, 5, 65, 300)] == [26, 36, 40, 50, 218, 760]
    # x = 0 is in the raw rows: (0, +-2) from the root, the identity from the chain
    rec, want = dict(gc.check_records()), dict(gc.check_expected())
    zero = [i for i, r in enumerate(rec["point_from_x"]) if not any(r[:12])]
    assert len(zero) == 2 and {tuple(want["point_from_x"][i][13:]) for i in zero} == {tuple(g1.mont_words(2)), tuple(g1.mont_words(g1.P - 2))}
    t = gc.torsion_points()
    assert {"identity", "(0, 2)", "(0, p - 2)", "order 11", "order 10177", "order dividing h", "subgroup 0", "generic 0"} <= set(t)
    assert g1.clear_cofactor(t["(0, 2)"]) is None and g1.clear_cofactor(t["order 11"]) is None and g1.clear_cofactor(t["generic 0"]) is not None
    edges = [sum(w << (32 * i) for i, w in enumerate(r)) for r in rec["fp_accept"][:len(gc.FP_EDGES)]]
    assert {g1.P - 1, g1.P, g1.P + 1, 0, (1 << 381) - 1, g1.P - (1 << 32), g1.P + (1 << 32)} <= set(edges) and any(e >> 381 for e in edges)


def test_twin_against_the_model(twin, tmp_path):
    assert gc.list_operations(twin) == gc.TABLE
    records = gc.check_records()
    got = gc.run_check(twin, records, tmp_path, "all")
    assert gc.assert_rows(records, got, gc.check_expected(), ("host twin", "model")) == sum(len(r) for _, r in records) > 250


def test_twin_under_sanitizers(tmp_path):
    """the twin built with -fsanitize=undefined,address (no recovery) as a stand-alone program: the shifts of the limb conversions and the
    addition chain's walk over small-order points are what this run is for"""
    exe = gc.build_host_twin(tmp_path, extra=["-O1", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"], name="rng_g1_check_san")
    records = gc.check_records()
    got = gc.run_check(exe, records, tmp_path, "san")
    assert gc.assert_rows(records, got, gc.check_expected(), ("sanitized twin", "model")) == sum(len(r) for _, r in records)


def test_the_check_notices_a_wrong_word(twin, tmp_path):
    records = gc.check_records()[2:]
    got = gc.run_check(twin, records, tmp_path, "two")
    bad = [(n, a.copy()) for n, a in got]
    bad[1][1][3, 5] ^= 1
    with pytest.raises(AssertionError, match="clear_cofactor row 3"):
        gc.assert_rows(records, bad, gc.check_expected()[2:], ("host twin", "model"))


@pytest.fixture(scope="module")
def lib():
    from curdleproofs_amd.build import build
    build()
    import curdleproofs_amd as cpx
    return cpx.load_library()


def test_names_everywhere(lib):
    import curdleproofs_amd as cpx
    hdr = open(os.path.join(ROOT, "include", "cpx.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "crs_mi355x.rs")).read()
    for name in NAMES:
        assert name in cpx.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, hdr), "include/cpx.h lacks %s" % name
        assert re.search(r"pub fn %s\(" % name, ffi), "integration/rust/ffi.rs lacks %s" % name
    assert "cpx_crs_generate(" in rs and "pub fn generate_crs(" in rs
    for k in KERNELS:
        assert k in cpx.Context.KERNELS and '"%s"' % k in hdr
    from curdleproofs_amd import build, crs, rng
    assert "rng_g1.hip" in build.SOURCES
    assert callable(crs.generate_crs) and callable(rng.g1_many) and callable(rng.instance_draws) and callable(rng.StdRng.g1)
    assert callable(cpx.Context.clear_cofactor)


def test_null_context_is_an_argument_error(lib):
    import curdleproofs_amd as cpx
    assert lib.cpx_rng_g1(None, 1, None, 1, None, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_rng_instance_draws(None, 1, None, None, None, None, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_crs_generate(None, 4, None, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_g1_clear_cofactor(None, None, 1, None) == cpx.CPX_ERR_ARG
    st = bytes(40)
    import ctypes
    buf = (ctypes.c_uint8 * 40).from_buffer_copy(st)
    assert lib.cpx_crs_generate(None, 4, buf, None) == cpx.CPX_ERR_ARG and bytes(buf) == st
