"""The quad-cooperative point formulas (curdleproofs_amd/csrc/g1_28_quad.hpp) and the work-group inversions (block_inverse.hpp) on
the GPU, on raw limbs: tests/device/quad_check.hip (built by curdleproofs_amd/build.py beside the library) runs xyzz28_add_quad_core,
xyzz28_add_quad_mem, xyzz28_dbl_quad, jac28_dbl_quad (alone and 1..120 times in a row in registers), a double-and-add ladder over LDS,
xyzz28_from_jac and block_batch_inverse / t_block_batch_inverse in work-groups of 64 and 256 over the rows of tests/quad_check_lib.py:
lazy representatives at the first and last value of every documented range, P + P and P - P on the same and on different ZZ, the
identity on either side and doubled, same-slot operands, exceptional additions in mid-chain, waves that hold all five outcomes of an
addition and waves that hold one, zero lanes at the ends of a work-group, in every second lane, in a whole wave and in all lanes.

Everything is exact integer arithmetic against Python integers and the oracle (tests/quad_check_lib.py says what is asserted); the
four lanes of a quad must agree bit for bit.  Nothing is skipped: the count of rows checked equals the count generated, the count of
values compared equals the count the integers expect (r of the core only under QUAD_OK, an inversion only where the lane is not zero).
One process of the check program per test, under a timeout; a non-zero exit fails the test at once and nothing is retried.  A failure
names the operation, the record, the row, the lane and the operand and result limbs."""
import os

import pytest

from tests import field_check_lib as fc
from tests import quad_check_lib as ql

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    from curdleproofs_amd.build import check_path
    assert os.path.exists(check_path("quad_check")), "run python -m curdleproofs_amd.build"
    return check_path("quad_check")


@pytest.fixture(scope="module")
def qv(orc):
    return ql.QuadVectors(orc)


@pytest.fixture(scope="module")
def checker(orc):
    return ql.Checker(fc.PointChecks(orc))


def _run(device, checker, tmp_path, records, tag):
    """one process over `records`; returns (rows checked, values compared) after asserting that no row was left out"""
    assert all(rows for _, rows in records)
    got = ql.run(device, records, tmp_path, tag, timeout=120)
    rows, compared = checker.check(records, got)
    assert rows == sum(len(r) for _, r in records)
    return rows, compared


def test_device_program_has_the_operation_table(device):
    assert ql.list_operations(device) == ql.TABLE


def test_additions(device, qv, checker, tmp_path):
    records = qv.add_records()
    assert [n for n, _ in records] == ["xyzz28_add_quad_core"] * 2 + ["xyzz28_add_quad_mem"] * 2
    rows, compared = _run(device, checker, tmp_path, records, "add")
    ok = sum(1 for n, rs in records[:2] for r in rs if ql.add_row_code(r) == ql.OK)
    assert ok > 0 and compared == ok + sum(len(rs) for _, rs in records[2:])      # r of the core is compared under QUAD_OK, and only there


def test_doublings(device, qv, checker, tmp_path):
    records = qv.dbl_records()
    assert {n for n, _ in records} == {"xyzz28_dbl_quad", "jac28_dbl_quad"}
    rows, compared = _run(device, checker, tmp_path, records, "dbl")
    assert compared == rows


def test_chains_and_ladder(device, qv, checker, tmp_path):
    records = qv.chain_records() + qv.ladder_records()
    assert {n for n, _ in records} == {"jac28_dbl_quad/chain", "xyzz28_quad_ladder"}
    rows, compared = _run(device, checker, tmp_path, records, "chain")
    assert compared == rows


def test_from_jac(device, qv, checker, tmp_path):
    rows, compared = _run(device, checker, tmp_path, qv.from_jac_records(), "from_jac")
    assert compared == rows


@pytest.mark.parametrize("name", list(ql.INVERSIONS))
def test_inversions(device, qv, checker, tmp_path, name):
    records = qv.inverse_records(name)
    n = ql.INVERSIONS[name]
    assert len(records[0][1]) == n * len(qv.inverse_blocks(name)) == n * (12 if n == 256 else 11)      # one work-group per pattern (the all-zero one must run to its end)
    rows, compared = _run(device, checker, tmp_path, records, "inverse")
    live = sum(1 for r in records[0][1] if any(r))
    assert 0 < live < rows and compared == live                      # a lane whose input is exact zero is unspecified: not compared
