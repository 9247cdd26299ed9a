"""CPU checks of the layout and the task lists of the verifier's accumulated check (curdleproofs_amd/csrc/check_plan.hpp): the ONE place
where the host-driven and the device-resident verifier decide where a proof's scalars sit, what its gather list is and what the MsmTask /
FixTask of the per-proof, the fused and the two stages of the grouped check look like.  Compiled with g++ into the stand-alone program
tests/host_emul/check_plan_emul.cpp, once plain and once with -fsanitize=address,undefined (the planner makes no HIP call; the HIP headers
are only needed for the task types of kernels.h), and compared with the same rules restated here in plain Python."""
import os
import subprocess

import pytest

from tests.check_harness import build_emul

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "curdleproofs_amd", "csrc")
OK, ERR_VERIFY, ERR_DESERIALIZE = 0, -4, -5
ELL, L = 28, 5
N = ELL + 4                                     # CRS scalars per proof
NI, NM = 4 * ELL, 6 + 18 + 10 * L               # R | S | T | U; the CRS singles and M (slots 0 .. 5), then the 18 + 10 L proof points
NPT = NI + NM
STRIDE = NPT + 19                               # entries per row of the per-proof points: more than the check reads
BATCHES = (1, 2, 10, 55, 56, 257, 600)
GROUPS_MAX = (1, 4, 256)
FIX_PARTS = (1, 8)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    exe = build_emul("check_plan_emul.cpp", ["include/cpx.h", "check_plan.hpp", "locate_plan.hpp", "layout.hpp", "kernels.h", "g1.hpp", "g1_28.hpp"], request.param == "sanitized")

    def run(B, groups_max, fix_parts, suspects):
        out = subprocess.run([exe] + [str(a) for a in (B, groups_max, ELL, L, fix_parts, STRIDE)] + ["".join(str(int(b)) for b in suspects)], check=True,
                             capture_output=True, text=True).stdout                        # a sanitizer report is a non-zero exit
        res = {"msm": {k: [] for k in ("proof", "groups", "fused", "suspects")}, "fix": {k: [] for k in ("proof", "groups", "fused", "suspects")}, "verdict": {}}
        for line in out.splitlines():
            key, *vals = line.split()
            if key in ("msm", "fix"):
                row = [v if v in "RGCS" else int(v) for v in vals[1:]]
                assert row[0] == len(res[key][vals[0]])                                    # numbered in order
                res[key][vals[0]].append(tuple(row[1:]))
            elif key == "verdict":
                res[key][(int(vals[0]), int(vals[1]))] = int(vals[2])
            else:
                res[key] = [int(v) for v in vals]
        return res
    return run


def grouping(B, groups_max):
    """locate_plan.hpp's rule: G = ceil(B / groups_max) proofs per group, NT = ceil(B / G) groups, the last one may be short"""
    G = -(-B // groups_max)
    return G, -(-B // G)


# ---- the rules, restated: a task as (bases, idx block, idx offset, scalars, n, flags, conv_off) / (idx is null, block, scalars, off, n, flags, out_first)
def proof_lists(B, fp):
    return ([(p * STRIDE, "R", 0, p * NPT, NPT, 0, p * NPT) for p in range(B)], [(1, "C", p * N, 0, N, 0, p * fp) for p in range(B)])


def group_msm(B, groups_max):
    G, NT = grouping(B, groups_max)
    return [(0, "G", g * G * NPT, g * G * NPT, min(G, B - g * G) * NPT, 0, g * G * NPT) for g in range(NT)]


def group_lists(B, groups_max, fp):
    return group_msm(B, groups_max), [(1, "S", g * N, 0, N, 0, g * fp) for g in range(grouping(B, groups_max)[1])]


def fused_lists(B):
    return group_msm(B, 256), [(1, "S", 0, 0, N, 0, 0)]


def suspect_lists(listed, fp):
    return ([(0, "G", p * NPT, p * NPT, NPT, 0, s * NPT) for s, p in enumerate(listed)], [(1, "C", p * N, 0, N, 0, s * fp) for s, p in enumerate(listed)])


# ---- what a list addresses, whatever its form
def point_range(task):
    """the task's points in the numbering of the batch (point i of proof p: p NPT + i)"""
    bases, blk, idx_off, _, n, _, _ = task
    if blk == "R":                                         # a row of the per-proof points through the row-relative list
        assert bases % STRIDE == 0 and idx_off == 0 and n == NPT
        return bases // STRIDE * NPT, n
    assert bases == 0
    return idx_off, n


def addressed(msm, gather):
    """(entry of the per-proof points, scalar) for every point of every task, in task order"""
    out = []
    for bases, blk, idx_off, scal, n, _, _ in msm:
        idx = range(n) if blk == "R" else gather[idx_off:idx_off + n]
        out += [(bases + i, scal + j) for j, i in enumerate(idx)]
    return out


def disjoint(ranges, limit):
    at = 0
    for first, count in sorted(ranges):
        assert first >= at and count > 0, ranges
        at = first + count
    assert at <= limit, (ranges, limit)


def check_list(msm, fix, B, fp, want_ranges, sum_rows):
    """the properties every list has: its tasks' point ranges are `want_ranges` in order; scalar, gather and conv_off ranges inside their
    buffers and disjoint between tasks; out_first ranges of width fix_parts disjoint"""
    assert [point_range(t) for t in msm] == want_ranges
    max_n = max([t[4] for t in msm], default=0)
    disjoint([(t[3], t[4]) for t in msm], B * NPT)                                         # scalars of the points
    disjoint([(t[2], t[4]) for t in msm if t[1] == "G"], B * NPT)                          # entries of the global gather list
    disjoint([(t[6], t[4]) for t in msm], len(msm) * max_n)                                # table-form scratch of the phase
    assert all(t[5] == 0 for t in msm) and all(t[5] == 0 and t[0] == 1 and t[3] == 0 and t[4] == N for t in fix)
    for blk, limit in (("C", B * N), ("S", sum_rows * N)):
        disjoint([(t[2], t[4]) for t in fix if t[1] == blk], limit)
    disjoint([(t[6], fp) for t in fix], len(fix) * fp)


@pytest.mark.parametrize("fix_parts", FIX_PARTS)
@pytest.mark.parametrize("groups_max", GROUPS_MAX)
@pytest.mark.parametrize("B", BATCHES)
def test_lists_match_the_rules(emul, B, groups_max, fix_parts):
    G, NT = grouping(B, groups_max)
    FG, FNT = grouping(B, 256)
    sparse = [p % 3 == 1 or p == B - 1 for p in range(B)]
    listed = [p for p in range(B) if sparse[p]]
    pl = emul(B, groups_max, fix_parts, sparse)
    assert pl["sizes"] == [NI, NM, NPT, B * NPT] and (NPT, N) == (186, 32)
    assert pl["plans"] == [G, NT, FG, FNT]
    gather = pl["gather"]
    assert gather == [p * STRIDE + i for p in range(B) for i in range(NPT)]
    per_proof = [(p * NPT, NPT) for p in range(B)]
    # per proof
    assert (pl["msm"]["proof"], pl["fix"]["proof"]) == proof_lists(B, fix_parts)
    check_list(pl["msm"]["proof"], pl["fix"]["proof"], B, fix_parts, per_proof, 0)
    # the groups of the plan: stage 1 of the grouped check
    assert (pl["msm"]["groups"], pl["fix"]["groups"]) == group_lists(B, groups_max, fix_parts)
    check_list(pl["msm"]["groups"], pl["fix"]["groups"], B, fix_parts, [(g * G * NPT, min(G, B - g * G) * NPT) for g in range(NT)], NT)
    assert sum(t[4] for t in pl["msm"]["groups"]) == B * NPT                                # ... which partition the batch's points
    if G == 1:
        assert addressed(pl["msm"]["groups"], gather) == addressed(pl["msm"]["proof"], gather)
        assert [t[6] for t in pl["msm"]["groups"]] == [t[6] for t in pl["msm"]["proof"]] and [t[6] for t in pl["fix"]["groups"]] == [t[6] for t in pl["fix"]["proof"]]
    # fused: the group tasks of the plan for 256 groups, entry for entry, and ONE fixed-base task over sums row 0
    assert (pl["msm"]["fused"], pl["fix"]["fused"]) == fused_lists(B)
    assert pl["msm"]["fused"] == emul(B, 256, fix_parts, sparse)["msm"]["groups"]
    check_list(pl["msm"]["fused"], pl["fix"]["fused"], B, fix_parts, [(g * FG * NPT, min(FG, B - g * FG) * NPT) for g in range(FNT)], 1)
    assert sum(t[4] for t in pl["msm"]["fused"]) == B * NPT and FNT <= 256
    # the suspects: stage 2, the listed proofs' ranges, dense slots
    assert (pl["msm"]["suspects"], pl["fix"]["suspects"]) == suspect_lists(listed, fix_parts)
    check_list(pl["msm"]["suspects"], pl["fix"]["suspects"], B, fix_parts, [(p * NPT, NPT) for p in listed], 0)
    by_proof = dict(zip(range(B), zip(pl["msm"]["proof"], pl["fix"]["proof"])))
    for (m, f), p in zip(zip(pl["msm"]["suspects"], pl["fix"]["suspects"]), listed):
        assert addressed([m], gather) == addressed([by_proof[p][0]], gather) and f[1:3] == by_proof[p][1][1:3]


@pytest.mark.parametrize("B", BATCHES)
def test_every_proof_suspect_is_the_per_proof_check(emul, B):
    fp = 8
    pl = emul(B, 4, fp, [1] * B)
    gather = pl["gather"]
    assert addressed(pl["msm"]["suspects"], gather) == addressed(pl["msm"]["proof"], gather)
    assert [t[1:5] for t in pl["fix"]["suspects"]] == [t[1:5] for t in pl["fix"]["proof"]]
    assert [t[6] for t in pl["msm"]["suspects"]] == [s * NPT for s in range(B)]               # dense conv_off
    assert [t[6] for t in pl["fix"]["suspects"]] == [s * fp for s in range(B)]
    check_list(pl["msm"]["suspects"], pl["fix"]["suspects"], B, fp, [(p * NPT, NPT) for p in range(B)], 0)


def test_the_verdict_rule_puts_decode_before_structural_before_the_check(emul):
    v = emul(1, 1, 1, [0])["verdict"]
    assert v == {(0, 1): OK, (0, 0): ERR_VERIFY,                                              # no flag: the check decides
                 (2, 1): ERR_VERIFY, (2, 0): ERR_VERIFY,                                      # structural rejection, whatever the sum
                 (1, 1): ERR_DESERIALIZE, (1, 0): ERR_DESERIALIZE,                            # undecodable, whatever else
                 (3, 1): ERR_DESERIALIZE, (3, 0): ERR_DESERIALIZE}


def test_the_header_is_hip_free_and_states_each_rule_once():
    src = open(os.path.join(CSRC, "check_plan.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "hip" not in code.replace('#include "kernels.h"', "")                              # no HIP call: only the task types
    for once in ("FixTask{", "SL_A +", "4 * ell"):
        assert code.count(once) == 1, once
    assert code.count("MsmTask{") == 2                                                        # a proof's row, or a range of the batch
    for f in ("engine.cpp", "engine_device.cpp"):
        text = open(os.path.join(CSRC, f)).read()
        assert "(B + 255) / 256" not in text and "6 + NPP" not in text, f
