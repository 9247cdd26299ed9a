"""CPU side of the MSM wave check (tests/device/msm_check.hip, run on the GPU by tests/test_gpu_msm_waves.py): the Python model of
tests/msm_check_lib.py is pinned to the oracle without any device code, the case sets of tests/msm_cases.py reach the edges they claim
(asserted from the model alone), the operation table covers every instantiation kernels.hip launches, and the program builds for gfx950."""
import os
import re
import subprocess

import pytest

from tests import msm_cases as mc
from tests import msm_check_lib as ml
from tests.msm_cases import NONE, NEG, TBW_CAP
from tests.scalar_cases import R, Z2
from tests.test_host_emul import emul, _b, _o   # noqa: F401  (the fixture that builds tests/host_emul)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "curdleproofs_amd", "csrc")
JAC = 144


def _fr(orc, v):
    return orc.fr_from_canonical_bytes((v % R).to_bytes(32, "little"))


def _real_case(orc, form, n, seed, slices=1):
    """a case over REAL tables: entry (c, i) = 2^(8c) P_i, the upper half of the copies z^2 times the lower (kernels.h); the two-copy
    table of the waves without shifted copies holds P and z^2 P.  Returns (case, pool of the table entries, bases, scalars)."""
    copies = mc.form_copies(form)
    half = copies // 2
    bases = orc.rng(seed).g1_affine(n)
    pts = b"".join(orc.g1_scale(bases, _fr(orc, (1 << (8 * (c % half))) * (Z2 if c >= half else 1))) for c in range(copies))
    scalars = mc.mixed_scalars(n, seed)
    case = dict(name="real%d" % n, form=form, slices=slices, tables=[list(range(copies * n))], tasks=[mc.task(scalars, [mc.seg(0, n)])], reaches="")
    return case, ml.Pool(orc, pts=pts), bases, scalars


def _recombine(orc, pool, case):
    """sum over all waves, sets and buckets of weight x bucket: (position + 1 + 64 for the upper set) x 2^64 for weight class 1 of the
    two-segment tables x 2^(8 wave) for the waves without shifted copies"""
    _, wpw, perwin, segs = mc.FORMS[case["form"]]
    pts, sc = [], []
    for m in ml.body_model(case):
        nsets = len(m["buckets"])
        for s in range(nsets):
            cls = (s >> 1 if nsets == 4 else (ml.wave_windows(wpw, perwin, m["wv"])[0] % 16) // 8) if segs == 2 else 0
            for pos, refs in enumerate(m["buckets"][s]):
                if refs:
                    pts.append(pool.sum([x[0] for x in refs]))
                    sc.append(_fr(orc, (64 * (s & 1) + pos + 1) << (64 * cls + (8 * m["wv"] if perwin else 0))))
    return orc.g1_msm_jac(b"".join(pts), b"".join(sc)) if pts else pool.ident


@pytest.mark.parametrize("form,n,slices", [("tblw/8", 1, 1), ("tblw/8", 33, 2), ("tblw/32", 70, 1), ("tblw2/4", 33, 1), ("tblw2/16", 70, 4), ("tblw/2,perwin", 33, 1),
                                           ("tblw/2,perwin", 70, 2)])
def test_model_equals_the_oracle_on_real_tables(orc, emul, form, n, slices):
    """The model stands alone: over real shifted tables its buckets, recombined with the bucket weights, the class weight 2^64 and the
    window weights, are the oracle's MSM; the host emulation of the kernels' algorithm (emul_msm_endo) gives the same point."""
    case, pool, bases, scalars = _real_case(orc, form, n, 100 + n, slices)
    sc = b"".join(_fr(orc, k) for k in scalars)
    want = orc.g1_msm(bases, sc, naive=True)
    assert orc.g1_eq_jac(_recombine(orc, pool, case), want)
    o = _o(JAC)
    emul.emul_msm_endo(_b(bases), _b(sc), n, 1 if mc.FORMS[form][2] else 0, o)
    assert orc.g1_eq_jac(bytes(o), want)


def test_digits_recombine_to_the_scalar():
    """integers only: sign x digit x 256^(w mod 16) x (z^2 for the q half) sums to k mod r for every scalar of the case sets"""
    for k in mc.mixed_scalars(200, 1) + mc.tie_scalars() + mc.random_scalars(200, 2) + mc.small_digit_scalars(50, lambda i: i % 127 + 1, 3):
        d, lo, hi = ml.split_digits(k)
        v = sum((-1 if (lo if w < 16 else hi) else 1) * d[w] * (1 << (8 * (w % 16))) * (Z2 if w >= 16 else 1) for w in range(32))
        assert v % R == k


def _find(cases, name, form):
    return next(c for c in cases if c["name"] == name and c["form"] == form)


def test_cases_reach_the_three_round_limits():
    cases = mc.tblw_cases()
    m = ml.body_model(_find(cases, "cap600", "tblw/32"))[0]
    assert [r["by"] for r in m["rounds"]] == ["cap", "cap", "ntot"] and [r["end"] for r in m["rounds"]] == [256, 512, 600]
    assert all(r["total"] <= TBW_CAP for r in m["rounds"]) and m["rounds"][0]["total"] + 2048 > TBW_CAP
    m = ml.body_model(_find(cases, "cap600", "tblw2/32"))[0]
    assert [r["by"] for r in m["rounds"]] == ["cap", "cap", "ntot"]
    for f in ("tblw/2", "tblw/32", "tblw2/16"):
        m = ml.body_model(_find(cases, "roundpts1089", f))[0]           # wave 0 holds window 0
        r0, r1 = m["rounds"]
        assert r0["by"] == "round_pts" and r0["end"] == 1024 and r0["total"] == 1024 and max(g for g, _, _, _ in r0["ents"]) == 1023
        assert max(e for l in r0["lists"] for e in l) >> 6 == 1023      # the 10-bit point index is used to its end
        # later rounds and empty bins: bin 76 is empty in round 1 and filled in round 2; round 2 leaves all bins but three empty while they
        # hold a parked accumulator from round 1
        assert r0["cnt"][76] == 0 and r1["cnt"][76] > 0
        assert sum(1 for b in range(128) if r1["cnt"][b] == 0 and r0["cnt"][b] > 0) >= 120
    for name in ("perwin4097", "perwin4097/digits"):
        for m in ml.body_model(_find(cases, name, "tblw/2,perwin")):
            r0, r1 = m["rounds"]
            assert r0["by"] == "round_pts" and r0["end"] == 4096 and r0["total"] <= TBW_CAP and r1["end"] == 4097
        assert max(e for l in r0["lists"] for e in l) >> 2 == 4095
    for n in (1, 63, 64, 65):
        m = ml.body_model(_find(cases, "n%d" % n, "tblw/4"))[0]
        assert [r["end"] for r in m["rounds"]] == [n]


def test_cases_reach_empty_slices_equal_windows_and_exceptional_buckets():
    cases = mc.tblw_cases()
    model = ml.body_model(_find(cases, "mixed100/s4", "tblw/2"))
    empty = [m for m in model if m["slice"] >= 2]
    assert len(empty) == 32 and all(m["first"] == m["ntot"] == 100 and not any(b for s in m["buckets"] for b in s) for m in empty)
    assert [(m["first"], m["ntot"]) for m in model[:2]] == [(0, 64), (64, 100)]
    model = ml.body_model(_find(cases, "mixed257/s2", "tblw/8"))
    assert [(m["first"], m["ntot"]) for m in model[:2]] == [(0, 192), (192, 257)]
    m = ml.body_model(_find(cases, "equal300", "tblw/32"))[0]
    assert all(r["cnt"][4] == r["total"] > 0 for r in m["rounds"]) and m["rounds"][0]["by"] == "cap"
    # buckets 0, 63, 64, 126 and 127 (the digits +-1, +-64, +-65, 127, -128) are reached, with both signs
    m = ml.body_model(_find(cases, "mixed100/s1", "tblw/32"))[0]
    for s, pos in ((0, 0), (0, 63), (1, 0), (1, 62), (1, 63)):
        assert m["buckets"][s][pos], (s, pos)
    # the zero scalar is there and reaches nothing
    assert 0 in _find(cases, "mixed100/s1", "tblw/32")["tasks"][0]["scalars"] and ml.split_digits(0)[0] == [0] * 32
    # exceptional additions: a bucket with the same point twice, one that holds P, P, -P and one more point, one that ends as the identity
    for f in mc.ALL_TBLW:
        model = ml.body_model(_find(cases, "exceptional", f))
        bs = [[x[0] for x in b] for m in model for s in m["buckets"] for b in s if b]
        assert any(len(b) == 5 and NONE in b and len({r & (NEG - 1) for r in b if r != NONE}) == 2 for b in bs), f
        assert any(sorted(r ^ NEG for r in b if r & NEG) == sorted(r for r in b if not r & NEG) for b in bs), f      # P and -P only: ends as the identity
        assert any(NONE not in b and not any(r & NEG for r in b) and len(set(b)) < len(b) for b in bs), f               # the same point twice
    # two segments: the boundary at 70 lies inside the second slab, both tables are wider than their segments
    for c in cases:
        if c["name"].startswith("seg70+50"):
            s0, s1 = c["tasks"][0]["segs"]
            assert (s0["n"], s1["n"]) == (70, 50) and s0["stride"] > s0["n"] and s1["stride"] > s1["n"]
    assert {(c["tasks"][0]["segs"][0]["idx"] is not None, c["tasks"][0]["segs"][1]["idx"] is not None) for c in cases if c["name"].startswith("seg70+50")} == {(True, False), (False, True), (True, True)}
    assert any(not c["tasks"][0]["canonical"] for c in cases)


def test_pair_cases_reach_every_rank_tie_and_a_far_longest_pair():
    cases = {c["name"]: c for c in mc.pair_cases()}
    model = ml.body_model(cases["pair/ties"])
    for m in model[:15]:                                             # waves 0..14: every bucket holds two entries per task
        cnt = m["rounds"][0]["cnt"]
        assert cnt == [2] * 128
        order = m["rounds"][0]["order"]
        assert len({cnt[order[l]] + cnt[order[127 - l]] for l in range(64)}) == 1
    m = ml.body_model(cases["pair/longest"])[3]
    cnt, order = m["rounds"][0]["cnt"], m["rounds"][0]["order"]
    sizes = sorted(cnt[order[l]] + cnt[order[127 - l]] for l in range(64))
    assert sizes[-1] >= 300 and sizes[-1] > 20 * sizes[-2]
    m = ml.body_model(cases["pair/mixed100"])
    assert len(m) == 32 and m[0]["slots"] != m[16]["slots"] and m[0]["slots"][2] - m[0]["slots"][0] == 107      # the second task's pad
    a, b = m[0]["buckets"][0], m[0]["buckets"][2]                    # sets 2, 3: the same addresses in the second task's table, other tags
    assert [[x[1:3] for x in y] for y in a] != [[x[1:3] for x in y] for y in b]
    assert [len(x) for x in a] == [len(x) for x in b]
    assert len(ml.body_model(cases["pair/n4097"])[0]["rounds"]) == 2


def test_part_slots_are_a_permutation_of_the_tasks_range():
    """the slots of a task's waves cover [pad, pad + sets) exactly once, the class-1 slots of the two-segment tables first"""
    for form, (kind, wpw, perwin, segs) in mc.FORMS.items():
        if kind == "pair":
            continue
        for slices in (1, 2, 4):
            waves = ml.n_waves(wpw, perwin)
            nsets = 4 if segs == 2 and wpw >= 16 else 2
            slots = {}
            for wv in range(waves):
                for sl in range(slices):
                    for s in range(nsets):
                        slots[ml.part_slot(wpw, segs, waves, slices, wv, sl, s)] = (wv, s)
            assert sorted(slots) == list(range(waves * slices * nsets)), (form, slices)
            if segs == 2:
                for slot, (wv, s) in slots.items():
                    cls = s >> 1 if nsets == 4 else (ml.wave_windows(wpw, perwin, wv)[0] % 16) // 8
                    assert (slot < len(slots) // 2) == (cls == 1), (form, slices, slot)


def test_operation_table_covers_what_the_library_launches():
    """every bucket-list and fixed-base instantiation on a CPX_LAUNCH line of kernels.hip has its operation, and every sort the bodies of
    those kernels instantiate (CACHE = two windows per wave without PERWIN; 256 bins for the two-segment waves of 16 and 32 windows)"""
    with open(os.path.join(CSRC, "kernels.hip")) as f:
        launches = [l for l in f if "CPX_LAUNCH(" in l and not l.lstrip().startswith("#define")]
    text = "".join(launches)
    ops = set()
    for w, p in re.findall(r"CPX_LAUNCH\(\(?k_msm_tblw<(\d+)(?:, (true|false))?>", text):
        ops.add("tblw/%s%s" % (w, ",perwin" if p == "true" else ""))
    ops |= {"tblw2/%s" % w for w in re.findall(r"CPX_LAUNCH\(k_msm_tblw2<(\d+)>", text)}
    ops |= {"pair"} if "CPX_LAUNCH(k_msm_tblw_pair" in text else set()
    ops |= {"fix/%s,%s" % f for f in re.findall(r"CPX_LAUNCH\(\(k_msm_fix<(\d+), (\d+)>\)", text)}
    assert len(ops) == 12 + 7
    assert ops == set(mc.FORMS) | set(mc.FIX_FORMS)
    assert "k_msm_fix_tblw" in text                                  # its bodies: msm_fix_body<16, 2> and msm_tblw_body<2, false>
    sorts = set()
    for form, (kind, wpw, perwin, segs) in mc.FORMS.items():
        sorts.add((wpw, perwin, 256 if segs == 2 and wpw >= 16 else 128))
    assert sorts == {(w, p, b) for w, p, b, _ in mc.SORTS.values()}
    assert {d for w, p, b, d in mc.SORTS.values() if p} == {False, True}     # PERWIN with task.digits and without
    for k in ("k_reduce_sets_wave", "k_reduce_sets<false>", "k_reduce_groups<false>", "k_reduce_sets<true>", "k_reduce_groups<true>", "k_finalize_ranges_wave",
              "k_finalize_ranges,", "k_msm_tail_wave<true>", "k_msm_tail<true>"):
        assert "CPX_LAUNCH(" + k in text, k
    assert set(ml.TABLE.values()) == set(ml.GROUPS) | {"pool"}
    for g, n in (("sort", 9), ("tblw", 11), ("pair", 1), ("fix", 7), ("reduce", 2), ("finalize", 4)):
        assert sum(1 for v in ml.TABLE.values() if v == g) == n


def test_every_form_has_cases():
    forms = {c["form"] for c in mc.tblw_cases()} | {c["form"] for c in mc.pair_cases()}
    assert forms == set(mc.FORMS)
    for f in mc.ALL_TBLW:       # slices 1, 2 or 4 where the form takes them
        assert {c["slices"] for c in mc.tblw_cases() if c["form"] == f} >= {1, 4}
    assert {c["slices"] for c in mc.tblw_cases()} == {1, 2, 4}
    for op in mc.FIX_FORMS:
        cb, wpw = mc.FIX_FORMS[op]
        case = mc.fix_cases(op)
        assert {t["n"] for t in case["tasks"]} >= {0, 1, 255, 256, 257, 13} and 13 % (64 // wpw)
        rows, waves = ml.fix_model(op, case)
        assert any(m == (1 << (cb - 1)) - 1 for _, m, _ in rows) and any(m == 0 for _, m, _ in rows)      # digits -2^(cb-1) and +-1
        assert any(t["idx"] is None and t["off"] for t in case["tasks"]) and {t["canonical"] for t in case["tasks"]} == {True, False}
        assert all(len(w["lanes"]) == 64 for w in waves)
        if cb == 19:
            assert all(not w["lanes"][63] for w in waves)              # the idle lane


def _model_output(pool, case):
    """the output record a device that agrees with the model would write"""
    import numpy as np
    model = ml.body_model(case)
    w = [len(model), len(model[0]["slots"]), 0, 0, 0] + [s for m in model for s in m["slots"]]
    for m in model:
        for st in m["buckets"]:
            for refs in st:
                live = [x[0] for x in refs if x[0] != NONE]
                w += ml.bytes_words(pool.sum(live)) + [0 if live else 1]
    return np.array(w, dtype="<u4")


def test_the_checks_notice_a_wrong_bucket_a_skipped_one_and_a_wrong_round(orc):
    """the comparison is not vacuous: a record written from the model passes; one bucket holding its neighbour's sum, a bucket left as
    poison, an unreached bucket that is a valid point instead of the identity, a touched guard set and a wrong raw_slot each fail, naming
    the form, the case, the wave, the set, the bucket and the table addresses; so does a sort record with two ranks of order[] exchanged"""
    pool = ml.Pool(orc, pts=orc.rng(5).g1_affine(64) * (mc.POOL // 64))
    case = mc.exceptional_case("exceptional", "tblw/8")
    good = _model_output(pool, case)
    assert ml.check_tblw(pool, case, good) == 4 * 2 * 64
    o = 5 + 8
    model = ml.body_model(case)
    full = next(e for e in range(64) if model[0]["buckets"][0][e])
    empty = next(e for e in range(64) if not model[0]["buckets"][0][e])
    other = next(e for e in range(64) if model[0]["buckets"][0][e] and e != full)
    for what, edit in (("not the sum of the table entries", lambda a: a.__setitem__(slice(o + 37 * full, o + 37 * full + 36), a[o + 37 * other:o + 37 * other + 36].copy())),
                       ("never written", lambda a: a.__setitem__(o + 37 * full + 36, 2)),
                       ("not the identity", lambda a: a.__setitem__(slice(o + 37 * empty, o + 37 * empty + 37), a[o + 37 * full:o + 37 * full + 37].copy())),
                       ("guard sets", lambda a: a.__setitem__(3, 1)),
                       ("raw_slot", lambda a: a.__setitem__(6, a[6] + 2))):
        bad = good.copy()
        edit(bad)
        with pytest.raises(AssertionError) as e:
            ml.check_tblw(pool, case, bad)
        assert what in str(e.value) and "tblw/8 case exceptional" in str(e.value), str(e.value)
        if what.startswith("not") or what.startswith("never"):
            assert "wave 0" in str(e.value) and "set 0 position" in str(e.value) and "table 0 element" in str(e.value) or what == "not the identity"
    op, (name, sc, first, ntot, _) = "sort/4,0,128", mc.sort_cases("sort/4,0,128")[0]
    w = [8, 3]
    for wv in range(8):
        rounds = ml.sort_rounds([ml.split_digits(k) for k in sc], ml.wave_windows(4, False, wv), False, 128, first, ntot)
        w.append(len(rounds))
        for rd in rounds:
            w += [rd["end"], rd["total"]] + rd["cnt"] + rd["cur"] + rd["order"] + [x for l in rd["lists"] for x in reversed(l)]
    import numpy as np
    assert ml.check_sort(op, name, sc, first, ntot, np.array(w, dtype="<u4")) == 8
    w[3 + 2 + 256], w[3 + 2 + 257] = w[3 + 2 + 257], w[3 + 2 + 256]
    with pytest.raises(AssertionError) as e:
        ml.check_sort(op, name, sc, first, ntot, np.array(w, dtype="<u4"))
    assert "order[] differs first at rank 0" in str(e.value) and "sort/4,0,128 case mixed100 wave 0" in str(e.value)


def test_device_program_is_built_for_gfx950_with_the_operation_table():
    """build() leaves _lib/msm_check beside the library (linked against it); its table is the one the tests drive.  The source passes the
    compiler's front end for the host and for gfx950 with the library's device flags."""
    from curdleproofs_amd import build as b
    assert os.path.exists(b.check_path("msm_check")), "run python -m curdleproofs_amd.build"
    assert ml.list_operations(b.check_path("msm_check")) == ml.TABLE
    with open(b.check_path("msm_check"), "rb") as f:
        assert b"gfx950" in f.read()
    subprocess.check_call([b._hipcc(), "--offload-arch=" + b.ARCH] + b.DEVICE_FLAGS + ["-fsyntax-only", b.check_source("msm_check")])
