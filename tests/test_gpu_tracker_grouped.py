"""GPU checks of the grouped and the fused check of tracker proofs (curdleproofs_amd.whisk.are_valid_whisk_tracker_proofs_grouped /
whisk_tracker_proofs_partial -> cpx_whisk_verify_tracker_proofs_grouped / _fused).  The data are the per-item suite's 37 items and nine
mutations (tests/test_gpu_tracker_batch.py); expected verdicts come from the oracle's is_valid_whisk_tracker_proof, expected recheck counts
from those verdicts and the grouping rule, the expected partial sum from the oracle's MSM over scalars this file computes on Python
integers with the challenge of tests/strobe_ref.Transcript — never from the library under test.  Sizes: 1, 8, 9, 28 and 37 items at 1, 4
and 256 groups put one item per group, several per group, a short last group and a single group on the two new kernels."""
import ctypes

import pytest

from tests.test_gpu_tracker_batch import BAD_POINT, BLINDER_ZERO, IDENTITY, K_MINUS_ONE, K_ONE, K_ZERO, MUTATED, N, R_ONE, Data, _answers

pytestmark = pytest.mark.gpu

R_ = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
VALID = [j for j in range(N) if j not in MUTATED]          # the 28 unmutated items
KEEP = 64 << 20
SCRATCH_BUFFERS = 33                                       # include/cpx.h: 21 buffers of the tier-0 set, 12 of the shuffle set


@pytest.fixture(scope="module")
def data(orc):
    return Data(orc)


@pytest.fixture(scope="module")
def weights(orc):
    """two non-zero weights per item (a_i || b_i, wire form), seeded"""
    w = orc.rng(777).fr(2 * N)
    assert all(w[32 * i:32 * (i + 1)] != bytes(32) for i in range(2 * N))
    return [w[64 * i:64 * (i + 1)] for i in range(N)]


def _ctx(**options):
    import curdleproofs_amd as cpx
    return cpx.Context(0, options=options)


def _expected_rechecks(want, groups_max):
    """the grouping rule on the oracle's answers: the unflagged items of the groups that hold an answer of 0; none with one item per group"""
    n = len(want)
    G = -(-n // min(max(groups_max, 1), 256))
    if G == 1:
        return 0
    return sum(sum(1 for w in want[g:g + G] if w != -1) for g in range(0, n, G) if 0 in want[g:g + G])


# ---- verdicts and recheck count ----
@pytest.mark.parametrize("strict", [0, 1], ids=["ark_0_4_infinity", "strict_infinity"])
@pytest.mark.parametrize("groups_max", [1, 4, 256])
def test_verdicts_and_recheck_count_match_the_oracle_on_all_37(data, weights, groups_max, strict):
    from curdleproofs_amd import whisk
    want = data.want[bool(strict)]
    c = _ctx(strict_infinity=strict, locate_groups_max=groups_max)
    try:
        res, rechecked = whisk.are_valid_whisk_tracker_proofs_grouped(c, data.vt, data.vc, data.vp, weights)
    finally:
        c.close()
    got = _answers(res)
    assert got == want, [(j, g, w) for j, (g, w) in enumerate(zip(got, want)) if g != w]
    assert rechecked == _expected_rechecks(want, groups_max)
    if groups_max == 4:           # 10 / 10 / 10 / 7: the mutated items 8..16 make groups 0 and 1 fail
        assert rechecked == (15 if strict else 16)
    if groups_max == 1:
        assert rechecked == (32 if strict else 33)


# ---- all-valid batches, launch counts ----
@pytest.mark.parametrize("groups_max", [4, 256])
@pytest.mark.parametrize("count", [1, 8, 9, 28])
def test_all_valid_batches_pass_stage_one(data, weights, count, groups_max):
    from curdleproofs_amd import whisk
    idx = VALID[:count]
    c = _ctx(locate_groups_max=groups_max)
    try:
        whisk.are_valid_whisk_tracker_proofs(c, data.vt[:1], data.vc[:1], data.vp[:1])     # (the context's first call decodes the generator)
        c.set_profiling(True)
        c.reset_stats()
        res, rechecked = whisk.are_valid_whisk_tracker_proofs_grouped(c, [data.vt[j] for j in idx], [data.vc[j] for j in idx], [data.vp[j] for j in idx],
                                                                      [weights[j] for j in idx])
        launches = {k: c.stat(k)["launches"] for k in ("k_tracker_relations", "k_tracker_gather", "k_tracker_check_scalars")}
    finally:
        c.close()
    assert res == [True] * count and rechecked == 0
    assert launches == {"k_tracker_relations": 0, "k_tracker_gather": 0, "k_tracker_check_scalars": 1}


def test_one_wrong_item_costs_one_gather_and_one_relations_launch(data, weights):
    from curdleproofs_amd import whisk
    idx = VALID[:11] + [10]                       # item 10: s + 1; 12 items in 4 groups of 3, the wrong one in the last
    assert data.want[False][10] == 0
    c = _ctx(locate_groups_max=4)
    try:
        whisk.are_valid_whisk_tracker_proofs(c, data.vt[:1], data.vc[:1], data.vp[:1])
        c.set_profiling(True)
        c.reset_stats()
        res, rechecked = whisk.are_valid_whisk_tracker_proofs_grouped(c, [data.vt[j] for j in idx], [data.vc[j] for j in idx], [data.vp[j] for j in idx],
                                                                      [weights[j] for j in idx])
        launches = {k: c.stat(k)["launches"] for k in ("k_tracker_relations", "k_tracker_gather", "k_tracker_check_scalars")}
    finally:
        c.close()
    assert res == [True] * 11 + [False] and rechecked == 3
    assert launches == {"k_tracker_relations": 1, "k_tracker_gather": 1, "k_tracker_check_scalars": 1}


def test_launch_count_does_not_depend_on_the_count(data, weights):
    from curdleproofs_amd import whisk
    import curdleproofs_amd as cpx
    c = _ctx(locate_groups_max=4)
    try:
        whisk.are_valid_whisk_tracker_proofs(c, data.vt[:1], data.vc[:1], data.vp[:1])
        c.set_profiling(True)
        seen = {}
        for count in (9, 37):
            c.reset_stats()
            whisk.are_valid_whisk_tracker_proofs_grouped(c, data.vt[:count], data.vc[:count], data.vp[:count], weights[:count])
            g = {k: c.stat(k)["launches"] for k in cpx.Context.KERNELS if k.startswith("k_")}
            c.reset_stats()
            whisk.whisk_tracker_proofs_partial(c, data.vt[:count], data.vc[:count], data.vp[:count], weights[:count])
            f = {k: c.stat(k)["launches"] for k in cpx.Context.KERNELS if k.startswith("k_")}
            seen[count] = (g, f)
    finally:
        c.close()
    assert seen[9] == seen[37]
    g, f = seen[9]
    assert g["k_tracker_check_scalars"] == 1 and g["k_tracker_gather"] == 1 and g["k_tracker_relations"] == 1 and g["k_decompress"] == 1
    assert f["k_tracker_check_scalars"] == 1 and f["k_tracker_gather"] == 0 and f["k_tracker_relations"] == 0


# ---- helpers on Python integers and the oracle's group ----
def _canon(pt):
    """the encoding the transcript hashes: a set infinity flag is the canonical infinity (strict_infinity = 0)"""
    return IDENTITY if pt[0] & 0x40 else pt


def _challenge(orc, tracker, commitment, proof):
    from tests.strobe_ref import Transcript
    gen = orc.g1_compress(orc.g1_generator())
    t = Transcript(b"whisk_opening_proof")
    for pt in (commitment, gen, tracker.k_r_G, tracker.r_G, proof[:48], proof[48:96]):       # whisk.rs:204-216
        t.append_message(b"tracker_opening_proof", _canon(pt))
    return t.get_and_append_challenge(b"tracker_opening_proof_challenge")[0]


def _fr(orc, v):
    return orc.fr_from_canonical_bytes((v % R_).to_bytes(32, "little"))


def _int(orc, wire):
    return int.from_bytes(orc.fr_to_canonical_bytes(wire), "little")


def _jac(aff):
    from curdleproofs_amd import params
    return aff + (bytes(48) if aff == bytes(96) else params.fp_to_wire(1))


def _expected_partial(orc, trackers, commitments, proofs, rands, want):
    """sum over the unflagged items of a (s G + c k_G - A) + b (s r_G + c k_r_G - B) as one oracle MSM; identity points are left out"""
    bases, scalars, gen_scalar = [], [], 0
    for t, kc, pf, w, ans in zip(trackers, commitments, proofs, rands, want):
        if ans == -1:
            continue
        a, b = _int(orc, w[:32]), _int(orc, w[32:])
        s, c = int.from_bytes(pf[96:], "little"), _challenge(orc, t, kc, pf)
        gen_scalar += a * s
        for pt, sc in ((kc, a * c), (pf[:48], -a), (t.r_G, b * s), (t.k_r_G, b * c), (pf[48:96], -b)):
            if _canon(pt) != IDENTITY:
                bases.append(orc.g1_decompress(pt))
                scalars.append(_fr(orc, sc))
    bases.append(orc.g1_generator())
    scalars.append(_fr(orc, gen_scalar))
    return orc.g1_msm(b"".join(bases), b"".join(scalars))


def test_the_reference_transcript_gives_the_proofs_challenge(data, orc):
    """pins _challenge: on a valid item  s G + c k_G == A  through the oracle's arithmetic"""
    j = 4
    assert data.want[False][j] == 1
    c = _challenge(orc, data.vt[j], data.vc[j], data.vp[j])
    s = int.from_bytes(data.vp[j][96:], "little")
    lhs = orc.g1_msm(orc.g1_generator() + orc.g1_decompress(data.vc[j]), _fr(orc, s) + _fr(orc, c))
    assert orc.g1_compress_jac(lhs) == data.vp[j][:48]


# ---- the weights bind ----
def _shifted_proof(orc, data, j, on_b, sign):
    """item j's proof with A (or B) replaced by A + sign G and s recomputed for the new challenge: relation 1 (or 2) is off by exactly
    - sign G, the other one holds"""
    gen = orc.g1_generator()
    k, beta = _int(orc, data.k[j]), _int(orc, data.b[j])
    pf = data.proofs[j]
    old = orc.g1_decompress(pf[48:96] if on_b else pf[:48])
    new = orc.g1_compress_jac(orc.g1_add_jac(_jac(old), _jac(orc.g1_scale(gen, _fr(orc, sign)))))
    pf = (pf[:48] + new if on_b else new + pf[48:96]) + bytes(32)
    c = _challenge(orc, data.trackers[j], data.commitments[j], pf)
    return pf[:96] + ((beta - c * k) % R_).to_bytes(32, "little")


@pytest.mark.parametrize("on_b", [False, True], ids=["pair_on_A", "pair_on_B"])
def test_the_weights_bind(data, weights, orc, on_b):
    """Items i and j of one group carry A_i + G and A_j - G: their errors are - G and + G.  Under EQUAL weights they cancel — the group's
    sum is the identity, which is why the weights must be independent — and under independent weights both come out CPX_ERR_VERIFY."""
    from curdleproofs_amd import whisk
    idx = VALID[8:20]                              # 12 valid items, none with an edge witness; groups of 3 at locate_groups_max = 4
    i, j = 1, 2
    assert idx[0] > R_ONE
    tr, kc = [data.trackers[p] for p in idx], [data.commitments[p] for p in idx]
    pf = [data.proofs[p] for p in idx]
    pf[i], pf[j] = _shifted_proof(orc, data, idx[i], on_b, 1), _shifted_proof(orc, data, idx[j], on_b, R_ - 1)
    for p in (i, j):
        assert orc.is_valid_whisk_tracker_proof(tr[p].to_bytes(), kc[p], pf[p]) == 0
    w = [weights[p] for p in idx]
    equal = list(w)
    equal[j] = equal[i]
    c = _ctx(locate_groups_max=4)
    try:
        res, rechecked = whisk.are_valid_whisk_tracker_proofs_grouped(c, tr, kc, pf, w)
        res_eq, rechecked_eq = whisk.are_valid_whisk_tracker_proofs_grouped(c, tr, kc, pf, equal)
        partial, n_invalid = whisk.whisk_tracker_proofs_partial(c, tr, kc, pf, w)
        is_id = c.sum_jac(partial)[1]
    finally:
        c.close()
    assert res == [p not in (i, j) for p in range(12)] and rechecked == 3
    assert n_invalid == 0 and not is_id
    assert res_eq == [True] * 12 and rechecked_eq == 0, "the pair is built to cancel under equal weights"


# ---- neighbours of a flagged item, edge witnesses ----
def test_neighbours_of_a_flagged_item_are_not_rechecked(data, weights):
    from curdleproofs_amd import whisk
    idx = VALID[:12]
    tr, kc, pf = [data.vt[p] for p in idx], [data.vc[p] for p in idx], [data.vp[p] for p in idx]
    kc[4] = BAD_POINT                              # group 1 of 4 (items 3, 4, 5): its only non-valid item does not decode
    c = _ctx(locate_groups_max=4)
    try:
        res, rechecked = whisk.are_valid_whisk_tracker_proofs_grouped(c, tr, kc, pf, [weights[p] for p in idx])
        pf[7] = pf[7][:40]                         # a wrong length is reported per item and never reaches the sums
        res2, rechecked2 = whisk.are_valid_whisk_tracker_proofs_grouped(c, tr, kc, pf, [weights[p] for p in idx])
    finally:
        c.close()
    assert _answers(res) == [-1 if p == 4 else 1 for p in range(12)] and rechecked == 0
    assert _answers(res2) == [-1 if p in (4, 7) else 1 for p in range(12)] and rechecked2 == 0


def test_edge_witnesses_pass_stage_one_in_one_group(data, weights):
    """k = 0, k = 1, k = r - 1, blinder = 0 and r = 1 carry identity points on every plane (k_G, k_r_G; A, B) and the generator as r_G"""
    from curdleproofs_amd import whisk
    idx = [K_ZERO, K_ONE, K_MINUS_ONE, BLINDER_ZERO, R_ONE]
    assert data.vc[K_ZERO] == IDENTITY and data.vt[K_ZERO].k_r_G == IDENTITY and data.vp[BLINDER_ZERO][:96] == IDENTITY * 2
    args = ([data.vt[p] for p in idx], [data.vc[p] for p in idx], [data.vp[p] for p in idx], [weights[p] for p in idx])
    c = _ctx(locate_groups_max=1)
    try:
        c.set_profiling(True)
        res, rechecked = whisk.are_valid_whisk_tracker_proofs_grouped(c, *args)
        relations = c.stat("k_tracker_relations")["launches"]
        ok = whisk.are_all_valid_whisk_tracker_proofs(c, *args)
    finally:
        c.close()
    assert res == [True] * 5 and rechecked == 0 and relations == 0 and ok is True


# ---- fused partial sum ----
def test_fused_partial_of_the_all_valid_batch_is_the_identity(data, weights):
    from curdleproofs_amd import whisk
    args = ([data.vt[p] for p in VALID], [data.vc[p] for p in VALID], [data.vp[p] for p in VALID], [weights[p] for p in VALID])
    c = _ctx()
    try:
        partial, n_invalid = whisk.whisk_tracker_proofs_partial(c, *args)
        is_id = c.sum_jac(partial)[1]
        ok = whisk.are_all_valid_whisk_tracker_proofs(c, *args)
        empty = whisk.whisk_tracker_proofs_partial(c, [], [], [])
    finally:
        c.close()
    assert n_invalid == 0 and is_id and partial[96:] == bytes(48) and ok is True
    assert empty[1] == 0 and empty[0][96:] == bytes(48)                     # count = 0: Z = 0


@pytest.mark.parametrize("strict", [0, 1], ids=["ark_0_4_infinity", "strict_infinity"])
def test_fused_partial_matches_the_oracle_msm_and_adds_over_halves(data, weights, orc, strict):
    from curdleproofs_amd import whisk
    want = data.want[bool(strict)]
    c = _ctx(strict_infinity=strict)
    try:
        partial, n_invalid = whisk.whisk_tracker_proofs_partial(c, data.vt, data.vc, data.vp, weights)
        h = 19
        p1, n1 = whisk.whisk_tracker_proofs_partial(c, data.vt[:h], data.vc[:h], data.vp[:h], weights[:h])
        p2, n2 = whisk.whisk_tracker_proofs_partial(c, data.vt[h:], data.vc[h:], data.vp[h:], weights[h:])
        both, both_id = c.sum_jac(p1 + p2)
        ok = whisk.are_all_valid_whisk_tracker_proofs(c, data.vt, data.vc, data.vp, weights)
    finally:
        c.close()
    assert n_invalid == want.count(-1) == n1 + n2
    expected = _expected_partial(orc, data.vt, data.vc, data.vp, weights, want)
    assert orc.g1_compress_jac(expected) != IDENTITY
    assert orc.g1_compress_jac(partial) == orc.g1_compress_jac(expected)
    assert orc.g1_compress_jac(both) == orc.g1_compress_jac(partial) and not both_id and ok is False


# ---- arguments ----
def test_arguments(data, weights, orc):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    count = 9
    tr, kc, pf = cpx._in(b"".join(t.to_bytes() for t in data.vt[:count])), cpx._in(b"".join(data.vc[:count])), cpx._in(b"".join(data.vp[:count]))
    good = b"".join(weights[:count])
    ell = 28
    crs = orc.generate_crs_points(ell)
    inst = orc.make_instance(ell, 0, crs)
    c = _ctx()
    try:
        L, h = c._L, c._h
        c.set_crs(ell, crs)
        c.load_batch(*(inst[k] * 2 for k in ("vec_R", "vec_S", "vec_T", "vec_U", "M")))
        before = c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2)
        st = (ctypes.c_int * count)(*([55] * count))
        n = ctypes.c_size_t(77)
        partial = (ctypes.c_uint8 * 144)(*([0xaa] * 144))
        inv = ctypes.c_int(66)
        # a zero weight or a weight >= r anywhere: CPX_ERR_ARG before anything is written
        for bad in (bytes(32), R_.to_bytes(32, "little"), b"\xff" * 32):
            for at in (0, 2 * count - 1):
                rnd = cpx._in(good[:32 * at] + bad + good[32 * (at + 1):])
                assert L.cpx_whisk_verify_tracker_proofs_grouped(h, count, tr, kc, pf, rnd, st, ctypes.byref(n)) == cpx.CPX_ERR_ARG
                assert L.cpx_whisk_verify_tracker_proofs_fused(h, count, tr, kc, pf, rnd, partial, ctypes.byref(inv)) == cpx.CPX_ERR_ARG
        assert list(st) == [55] * count and n.value == 77 and bytes(partial) == b"\xaa" * 144 and inv.value == 66
        rnd = cpx._in(good)
        # NULL with work to do
        assert L.cpx_whisk_verify_tracker_proofs_grouped(h, count, tr, kc, pf, None, st, None) == cpx.CPX_ERR_ARG
        assert L.cpx_whisk_verify_tracker_proofs_grouped(h, count, tr, kc, pf, rnd, None, None) == cpx.CPX_ERR_ARG
        assert L.cpx_whisk_verify_tracker_proofs_fused(h, count, None, kc, pf, rnd, partial, ctypes.byref(inv)) == cpx.CPX_ERR_ARG
        assert L.cpx_whisk_verify_tracker_proofs_fused(h, count, tr, kc, pf, rnd, None, ctypes.byref(inv)) == cpx.CPX_ERR_ARG
        # more than 2^21 items: refused without reading the (far too small) buffers
        assert L.cpx_whisk_verify_tracker_proofs_grouped(h, (1 << 21) + 1, tr, kc, pf, rnd, st, None) == cpx.CPX_ERR_ARG
        assert L.cpx_whisk_verify_tracker_proofs_fused(h, (1 << 21) + 1, tr, kc, pf, rnd, partial, ctypes.byref(inv)) == cpx.CPX_ERR_ARG
        assert list(st) == [55] * count and bytes(partial) == b"\xaa" * 144 and inv.value == 66
        # count = 0: a no-op
        assert L.cpx_whisk_verify_tracker_proofs_grouped(h, 0, None, None, None, None, None, None) == cpx.CPX_OK
        assert L.cpx_whisk_verify_tracker_proofs_fused(h, 0, None, None, None, None, partial, ctypes.byref(inv)) == cpx.CPX_OK
        assert inv.value == 0 and bytes(partial)[96:] == bytes(48)
        # the calls themselves, n_rechecked NULL; the loaded batch, the CRS and the scratch contract
        assert L.cpx_whisk_verify_tracker_proofs_grouped(h, count, tr, kc, pf, rnd, st, None) == cpx.CPX_OK
        assert [1 if v == cpx.CPX_OK else 0 if v == cpx.CPX_ERR_VERIFY else -1 for v in st] == data.want[False][:count]
        assert L.cpx_whisk_verify_tracker_proofs_fused(h, count, tr, kc, pf, rnd, partial, ctypes.byref(inv)) == cpx.CPX_OK
        assert inv.value == 0
        assert c.batch == 2
        assert c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2) == before == [cpx.CPX_OK] * 2
        assert c.crs_sums() == orc.crs_sums(ell, crs)
        assert 0 < c.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    finally:
        c.close()
    fresh = _ctx()                                                          # no CRS, nothing loaded
    try:
        res, rechecked = whisk.are_valid_whisk_tracker_proofs_grouped(fresh, data.vt[:3], data.vc[:3], data.vp[:3], weights[:3])
        assert _answers(res) == data.want[False][:3] and rechecked == 0 and fresh.batch == 0
        res, rechecked = whisk.are_valid_whisk_tracker_proofs_grouped(fresh, data.vt[:3], data.vc[:3], data.vp[:3])      # weights from the CSPRNG
        assert _answers(res) == data.want[False][:3]
    finally:
        fresh.close()
