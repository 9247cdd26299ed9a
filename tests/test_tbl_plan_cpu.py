"""CPU checks of the planner of a table-backed MSM phase (curdleproofs_amd/csrc/tbl_plan.hpp): the ONE place where the host-driven
phases and the device-resident plans turn a list of requests into tasks of k_msm_fix / k_msm_tblw and the per-request ranges of
k_finalize_ranges.  Compiled with the host compiler by tests/host_emul/tbl_plan_emul.cpp (the planner makes no HIP call; the HIP
headers are only needed for the task types of kernels.h)."""
import ctypes
import random

import pytest

from tests.check_harness import build_emul

NONE, CRS, TAB = 0, 1, 2


@pytest.fixture(scope="module")
def planner():
    L = ctypes.CDLL(build_emul("tbl_plan_emul.cpp", ["tbl_plan.hpp", "kernels.h", "host_math.hpp", "g1.hpp", "g1_28.hpp"], shared=True))
    L.emul_tbl_plan.restype = ctypes.c_int
    return L


def _plan(L, reqs, fix, fix_parts, tbl_parts, dummy):
    nt = len(reqs)
    desc = (ctypes.c_uint32 * (6 * nt + 1))(*[x for r in reqs for x in r])
    counts, tt, ft = (ctypes.c_uint64 * 11)(), (ctypes.c_uint64 * (4 * nt + 4))(), (ctypes.c_uint64 * (8 * nt + 4))()
    meta, soff = (ctypes.c_uint32 * (6 * nt + 1))(), (ctypes.c_uint64 * (nt + 1))()
    differs = L.emul_tbl_plan(nt, desc, int(fix), fix_parts, tbl_parts, dummy, counts, tt, ft, meta, soff)
    keys = ("nt", "ntt", "nft", "nparts", "fix_sets", "tbl_sets", "nscal", "tbl_max_n", "any_add", "pts_fix", "pts_tbl")
    c = dict(zip(keys, counts))
    tasks_t = [tuple(tt[4 * k:4 * k + 4]) for k in range(c["ntt"])]
    tasks_f = [tuple(ft[4 * k:4 * k + 4]) for k in range(c["nft"])]
    return c, tasks_t, tasks_f, list(meta)[:6 * nt], list(soff)[:nt], differs


def _check(L, reqs, fix, fix_parts, tbl_parts):
    dummy = 77
    nt = len(reqs)
    c, tasks_t, tasks_f, meta, soff, differs = _plan(L, reqs, fix, fix_parts, tbl_parts, dummy)
    assert differs == 0, "the device form before sorting differs from the host form"
    first, count, dst, add = meta[:nt], meta[nt:2 * nt], meta[2 * nt:3 * nt], meta[3 * nt:]
    is_crs = lambda kind, n: fix and kind == CRS and n > 0
    # the ranges are disjoint and cover [0, nparts) in request order
    at = 0
    for i in range(nt):
        assert first[i] == at
        at += count[i]
    assert at == c["nparts"] == c["fix_sets"] + c["tbl_sets"]
    assert c["fix_sets"] == c["nft"] * fix_parts and c["tbl_sets"] == c["ntt"] * tbl_parts
    assert c["nt"] == nt and c["nscal"] == sum(r[1] + r[3] for r in reqs)
    assert c["any_add"] == int(any(r[4] for r in reqs))
    it = jf = off = 0
    max_n = pts_fix = pts_tbl = 0
    for i, (k0, n0, k1, n1, addend, has_dst) in enumerate(reqs):
        assert soff[i] == off
        f0, f1 = is_crs(k0, n0), is_crs(k1, n1)
        needs_tbl = (not fix) or (n0 > 0 and not f0) or (n1 > 0 and not f1)
        slot = first[i]
        if needs_tbl:   # the table task first ...
            pad, scal, s0n, s1n = tasks_t[it]
            it += 1
            assert pad == slot and first[i] <= pad < first[i] + count[i]
            assert scal == off + (n0 if f0 else 0)          # seg0 went to the fixed-base kernel: its scalars are skipped
            assert (s0n, s1n) == ((0 if f1 else n1, 0) if f0 else (n0, 0 if f1 else n1))
            max_n = max(max_n, s0n + s1n)
            pts_tbl += s0n + s1n
            slot += tbl_parts
        for f, n, at_scal, which in ((f0, n0, off, 0), (f1, n1, off + n0, 1)):   # ... then the fixed-base tasks
            if not f:
                continue
            out_first, scal, col, fn = tasks_f[jf]
            jf += 1
            assert out_first == slot and first[i] <= out_first < first[i] + count[i]
            assert (scal, col, fn) == (at_scal, i % 7 + which, n)
            pts_fix += n
            slot += fix_parts
        assert slot == first[i] + count[i]
        assert dst[i] == (2000 + i if has_dst else dummy)
        assert add[3 * i:3 * i + 3] == [1000 + i if addend else 0xffffffff, 0xffffffff, 0xffffffff]
        off += n0 + n1
    assert it == c["ntt"] and jf == c["nft"]
    assert (c["tbl_max_n"], c["pts_fix"], c["pts_tbl"]) == (max_n, pts_fix, pts_tbl)
    return c


MIXED = [
    (CRS, 256, NONE, 0, 0, 1),      # CRS only
    (TAB, 256, NONE, 0, 0, 0),      # table only
    (TAB, 128, TAB, 1, 0, 0),       # both segments on tables
    (CRS, 1, TAB, 1, 1, 1),         # first segment CRS (the prover's B = A + alpha M + beta sum(G)), with an addend
    (NONE, 0, NONE, 0, 1, 1),       # empty, addend-carrying (A')
    (CRS, 128, CRS, 1, 0, 0),       # both segments CRS (the IPA cross terms + the H term)
    (TAB, 5, CRS, 2, 0, 1),         # second segment CRS
    (NONE, 0, NONE, 0, 0, 0),       # empty
    (CRS, 2, NONE, 0, 1, 0),
]


@pytest.mark.parametrize("fix_parts,tbl_parts", [(1, 2), (2, 4), (8, 32), (16, 64)])
def test_planner_layout_of_a_mixed_request_list(planner, fix_parts, tbl_parts):
    c = _check(planner, MIXED, True, fix_parts, tbl_parts)
    assert (c["ntt"], c["nft"]) == (4, 6)


def test_planner_without_a_table_of_multiples_sends_every_request_to_the_table_kernel(planner):
    c = _check(planner, MIXED, False, 0, 4)
    assert (c["ntt"], c["nft"], c["fix_sets"]) == (len(MIXED), 0, 0)


def test_planner_layout_of_random_request_lists(planner):
    rnd = random.Random(9)
    for _ in range(200):
        reqs = []
        for _ in range(rnd.randrange(0, 40)):
            k0, k1 = rnd.choice((NONE, CRS, TAB)), rnd.choice((NONE, NONE, CRS, TAB))
            reqs.append((k0, rnd.choice((1, 2, 128, 255)) if k0 else 0, k1, rnd.choice((1, 3, 64)) if k1 else 0, rnd.randrange(2), rnd.randrange(2)))
        _check(planner, reqs, rnd.randrange(4) > 0, rnd.choice((1, 2, 4, 8)), rnd.choice((2, 4, 8, 16, 32, 64)))
