"""The gfx950 build of the scalar-side headers, function by function on raw words: tests/device/scalar_check.hip, built by
curdleproofs_amd/build.py beside the library, runs the endomorphism split, every signed-digit and non-adjacent recoding, the table
picks of the generator table and of the tracker ladder, one batch of division steps and every inversion in a kernel of its own over the
rows of tests/scalar_cases.py: the sign turns of k and t, t = 0 and q = 0, every window at and one below its carry threshold, the
alternating patterns with the longest carry runs, 2^b and 2^b - 1, the inversion inputs with the most batches.  Every row of the device
output must
  1. equal the host twin's output (the same source through g++) bit for bit, and
  2. pass the integer checks of tests/scalar_check_lib.py (Python integers and the documented contracts), which do not involve the twin.
No row is skipped: the counts of rows compared and checked equal the count generated.  A failure names the operation, the row and the
input words."""
import os

import pytest

from tests import scalar_check_lib as sl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return sl.build_host_twin(tmp_path_factory.mktemp("scalar_check"))


@pytest.fixture(scope="module")
def device():
    from curdleproofs_amd.build import check_path
    assert os.path.exists(check_path("scalar_check")), "run python -m curdleproofs_amd.build"
    return check_path("scalar_check")


def test_device_program_has_the_operation_table(device):
    assert sl.list_operations(device) == sl.TABLE


@pytest.mark.parametrize("group", sl.GROUPS)
def test_device_matches_host_twin_and_integers(device, twin, tmp_path, group):
    records = sl.group_records(group)
    assert {n for n, _ in records} >= {n for n in sl.TABLE if sl.group_of(n) == group}
    total = sum(len(rows) for _, rows in records)
    dev = sl.run(device, records, tmp_path, group + "_device", timeout=120)      # one process, one short kernel per operation
    host = sl.run(twin, records, tmp_path, group + "_host", timeout=600)
    assert sl.assert_same(records, dev, host) == total
    assert sl.check_integers(records, dev) == total
    assert sl.check_across(records, dev) == sl.across_count(group, records)
