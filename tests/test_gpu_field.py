"""The gfx950 build of the field and point headers, operation by operation on raw limbs: tests/device/field_check.hip, built by
curdleproofs_amd/build.py beside the library, runs every operation of mont32.hpp (the inline-assembly Montgomery product of the device
branch among them), fp28.hpp and g1_28.hpp in a kernel of its own over the operand sets of tests/f28_vectors.py: limbs at
+-(2^28 - 1), the top limb at 38 p, lazy differences and negations, Montgomery digits all 0 or all ones, carries into the third
accumulator word in the first and the last column, exceptional point operands.  Every row of the device output must
  1. equal the host twin's output (the same source through g++) bit for bit, and
  2. pass the integer checks of tests/field_check_lib.py (Python integers; the oracle for points), which do not involve the twin.
No row is skipped: the counts of rows compared and checked equal the count generated.  A failure names the operation, its body, the
row and the operand limbs."""
import os

import pytest

from tests import field_check_lib as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return fc.build_host_twin(tmp_path_factory.mktemp("field_check"))


@pytest.fixture(scope="module")
def device():
    from curdleproofs_amd.build import check_path
    assert os.path.exists(check_path("field_check")), "run python -m curdleproofs_amd.build"
    return check_path("field_check")


def test_device_program_has_the_operation_table(device):
    assert fc.list_operations(device) == fc.TABLE


@pytest.mark.parametrize("group", fc.GROUPS)
def test_device_matches_host_twin_and_integers(device, twin, orc, tmp_path, group):
    records = fc.group_records(group, orc)
    assert {n for n, _ in records} == {n for n in fc.TABLE if fc.group_of(n) == group}
    total = sum(len(rows) for _, rows in records)
    dev = fc.run(device, records, tmp_path, group + "_device", timeout=120)      # one process, one short kernel per operation
    host = fc.run(twin, records, tmp_path, group + "_host", timeout=600)
    assert fc.assert_same(records, dev, host) == total
    assert fc.check_integers(records, dev, fc.PointChecks(orc)) == total
