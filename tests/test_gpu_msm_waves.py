"""The MSM wave bodies of curdleproofs_amd/csrc/msm_body.hpp and the library's set reducers on the GPU, bucket by bucket:
tests/device/msm_check.hip (built by curdleproofs_amd/build.py beside the library) wraps tbw_sort, msm_tblw_body in every form the
library launches and msm_fix_body in kernels of its own, and calls the library's launch_reduce_sets, launch_finalize_ranges and
launch_msm_tail on crafted inputs.  The reference is the Python model of tests/msm_check_lib.py over TAGGED tables (every table entry
a point unrelated to every other, tests/msm_cases.py) and the oracle:
  sort      end, cnt[], cur[], order[] and every list of every round, exactly (the order inside a list is free);
  tblw/pair every bucket of every set of every wave as a group element, buckets nothing reaches as the identity itself, raw_slot, and
            the poisoned guard sets around the raw sets;
  fix       every lane of every wave likewise;
  reduce    plain, lower and upper sets through both kernel families against sum weight x entry;
  finalize  points and compressed bytes of k_finalize_ranges / _wave, the Horner tail in both forms.
No bucket is skipped: the number compared equals waves x sets x 64.  One process of the check program per test, under a timeout; a nonzero
exit fails the test at once and nothing is retried.  A failure names the operation, the case, the wave, the round or set, the bucket
and the table addresses the model expected there."""
import os

import pytest

from tests import msm_cases as mc
from tests import msm_check_lib as ml

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    from curdleproofs_amd.build import check_path
    assert os.path.exists(check_path("msm_check")), "run python -m curdleproofs_amd.build"
    return check_path("msm_check")


@pytest.fixture(scope="module")
def pool(orc):
    return ml.Pool(orc)


def test_device_program_has_the_operation_table(device):
    assert ml.list_operations(device) == ml.TABLE


def test_sort(device, tmp_path):
    cases = [(op,) + c for op in mc.SORTS for c in mc.sort_cases(op)]
    assert {op for op, *_ in cases} == {op for op, g in ml.TABLE.items() if g == "sort"}
    out = ml.run(device, [ml.sort_record(op, sc, first, ntot, canon) for op, _, sc, first, ntot, canon in cases], tmp_path, "sort")
    rounds = sum(ml.check_sort(op, name, sc, first, ntot, a) for (op, name, sc, first, ntot, _), a in zip(cases, out))
    assert rounds >= len(cases)


def _run_waves(device, pool, tmp_path, cases, tag):
    out = ml.run(device, [pool.record()] + [ml.tblw_record(c) for c in cases], tmp_path, tag, timeout=300)
    assert int(out[0][0, 0]) == mc.POOL
    n = sum(ml.check_tblw(pool, c, a) for c, a in zip(cases, out[1:]))
    want = 0
    for c in cases:
        kind, wpw, perwin, segs = mc.FORMS[c["form"]]
        want += (len(c["tasks"]) // (2 if kind == "pair" else 1)) * ml.n_waves(wpw, perwin) * c["slices"] * (4 if kind == "pair" or (segs == 2 and wpw >= 16) else 2) * 64
    assert n == want            # the compared count equals the generated count


def test_tblw(device, pool, tmp_path):
    cases = mc.tblw_cases()
    assert {c["form"] for c in cases} == {op for op, g in ml.TABLE.items() if g == "tblw"}
    _run_waves(device, pool, tmp_path, cases, "tblw")


def test_pair(device, pool, tmp_path):
    _run_waves(device, pool, tmp_path, mc.pair_cases(), "pair")


def test_fix(device, pool, tmp_path):
    cases = [(op, mc.fix_cases(op)) for op in mc.FIX_FORMS]
    out = ml.run(device, [pool.record()] + [ml.fix_record(op, c) for op, c in cases], tmp_path, "fix", timeout=300)
    n = sum(ml.check_fix(pool, op, c, a) for (op, c), a in zip(cases, out[1:]))
    assert n == sum(len(c["tasks"]) * ((-(-256 // mc.FIX_FORMS[op][0])) // mc.FIX_FORMS[op][1]) * 64 for op, c in cases)


def test_reduce(device, pool, tmp_path):
    case = ml.reduce_case()
    ops = ("reduce/wave", "reduce/sets")
    out = ml.run(device, [pool.record()] + [ml.reduce_record(op, case) for op in ops], tmp_path, "reduce")
    for op, a in zip(ops, out[1:]):
        assert ml.check_reduce(pool, op, case, a) == len(case[2])


def test_finalize(device, pool, tmp_path):
    fcs = [ml.finalize_case(pool, n) for n in (1, 64, 65)]
    tcs = [ml.tail_case(pool, 3, 16, 8, 2, 0), ml.tail_case(pool, 2, 16, 8, 8, 5), ml.tail_case(pool, 65, 4, 8, 1, 2), ml.tail_case(pool, 1, 1, 8, 4, 64)]
    recs = [ml.finalize_record(op, fc) for fc in fcs for op in ("finalize/wave", "finalize/ranges")]
    recs += [ml.tail_record(op, tc) for tc in tcs for op in ("tail/wave", "tail/lanes")]
    out = ml.run(device, recs, tmp_path, "finalize")
    i = 0
    for fc in fcs:
        for op in ("finalize/wave", "finalize/ranges"):
            assert ml.check_finalize(op, fc, out[i]) == fc["n"]
            i += 1
    for tc in tcs:
        for op in ("tail/wave", "tail/lanes"):
            assert ml.check_tail(pool, op, tc, out[i]) == tc["nout"]
            i += 1
