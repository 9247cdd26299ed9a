"""The gfx950 build of the three transcript implementations at every position of the rate: tests/device/transcript_check.hip, built
by curdleproofs_amd/build.py beside the library, runs WaveStrobe (wave_strobe.hpp: from global memory and from LDS), LaneStrobe
(lane_strobe.hpp) and the device build of cpx::Strobe (strobe.hpp) over the case sets of tests/transcript_cases.py: the permutation
from every single-bit state, every operation from every start position (every split of a scalar, of a length tail and of the header
bytes by the rate boundary), the product's own streams at message offsets 0..8, and challenges that retry once and twice.  Every case
of every engine must equal
  1. tests/strobe_ref.py (plain Python, pinned against the oracle by tests/test_transcript_check_cpu.py) and
  2. the host twin (the same source through g++)
word for word: the 25 state words, pos, pos_begin, every challenge and its attempt count.  No case is skipped: the counts compared
equal the count generated.  A failure names the engine, the case, the operation index, the start pos and the first differing word."""
import os

import pytest

from tests import strobe_ref as sr
from tests import transcript_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return tc.build_host_twin(tmp_path_factory.mktemp("transcript_check"))


@pytest.fixture(scope="module")
def device():
    from curdleproofs_amd.build import check_path
    assert os.path.exists(check_path("transcript_check")), "run python -m curdleproofs_amd.build"
    return check_path("transcript_check")


@pytest.fixture(scope="module")
def host_results(twin, tmp_path_factory):
    """the host twin's answers, once per set"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = tc.run_engine(twin, "strobe_host", tc.cases_of(name), tmp_path_factory.mktemp("host_" + name), name, timeout=600)
        return cache[name]
    return get


def test_device_program_has_the_operation_table(device):
    assert tc.list_operations(device) == tc.DEVICE_TABLE


@pytest.mark.parametrize("name", tc.SETS)
@pytest.mark.parametrize("engine", tc.DEVICE_ENGINES + ("strobe_host",))
def test_engine_equals_the_reference_and_the_host_twin(device, host_results, orc, tmp_path, engine, name):
    cases, want = tc.cases_of(name), tc.expected(name, orc)
    assert cases
    got = tc.run_engine(device, engine, cases, tmp_path, engine + "_" + name, timeout=120)      # one process, one kernel
    permute = sr.keccak_f1600 if name == "permutation" else tc.oracle_permute(orc)

    def locate(c):
        return tc.first_bad_operation(device, engine, c, permute, tmp_path)
    assert tc.assert_same(engine, cases, got, want, locate=locate) == len(cases)
    assert tc.assert_same(engine, cases, got, host_results(name), who="the host twin", locate=locate) == len(cases)


def test_bit_helpers_on_the_device(device, twin, tmp_path):
    records = tc.helper_records()
    got = tc.run_rows(device, records, tmp_path, "helpers")
    assert tc.check_helpers(got) == 2 * sum(len(r) for _, r in records[::2])
    tc.check_helper_round_trips(device, records, got, tmp_path)
    host = tc.run_rows(twin, records, tmp_path, "helpers_host")
    assert all((a == b).all() for (_, a), (_, b) in zip(got, host))
