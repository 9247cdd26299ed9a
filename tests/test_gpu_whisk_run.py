"""GPU tests of the Whisk shuffle run against the resident candidate list (cpx_whisk_candidates_load / _size / _read,
cpx_whisk_verify_shuffle_run and its grouped form, and their Python mirrors).  Expected verdicts and bytes come from the oracle and from a
plain Python replay of the list, never from the library under test.  ell = 28, 40 candidates and a run of 14 items: every item touches 28
of the 40 indices, so nearly every read hits an earlier write; 14 * 28 = 392 points are 13 work-groups of the copy kernels with dead
lanes in the last one.  The Whisk size ell = 124 runs once."""
import ctypes
import random

import pytest

pytestmark = pytest.mark.gpu

ELL = 28
NC = 40
NI = 14


def _bad_point(orc):
    """a compressed encoding whose x is the x of no curve point: the decoder's MALFORMED"""
    from tests import decoding_ref as dr
    x = next(x for x in range(1, 64) if not dr.is_qr(x ** 3 + 4))
    enc = dr.encode(x, 0x80)
    assert dr.decode(enc, orc)[0] == dr.MALFORMED
    return enc


def _cat(ts):
    return b"".join(t.to_bytes() for t in ts)


def _trackers(blob):
    from curdleproofs_amd import whisk
    return [whisk.WhiskTracker(blob[96 * j:96 * j + 48], blob[96 * j + 48:96 * j + 96]) for j in range(len(blob) // 96)]


def _chunks(blob, size):
    return [blob[i:i + size] for i in range(0, len(blob), size)]


def _wire(orc, vec_a, vec_b):
    """affine points (96 bytes each) -> one 96-byte tracker (r_G, k_r_G compressed) per pair"""
    ca, cb = orc.g1_compress(vec_a), orc.g1_compress(vec_b)
    return [ca[48 * j:48 * (j + 1)] + cb[48 * j:48 * (j + 1)] for j in range(len(ca) // 48)]


def replay_bytes(cand, tables, posts, upto=None):
    """The list after items 0 .. upto-1 (all of them: None) were written back, and the pre trackers every item reads when all its
    predecessors were written back.  Plain Python on 96-byte strings."""
    lst, pres = list(cand), []
    for b, (row, post) in enumerate(zip(tables, posts)):
        if upto is not None and b >= upto:
            break
        pres.append(b"".join(lst[i] for i in row))         # an item reads before it writes
        for j, i in enumerate(row):                        # rising j: the highest slot wins
            lst[i] = post[96 * j:96 * (j + 1)]
    return lst, pres


class Run:
    """A candidate list and a run of shuffles over it, proved item by item by the oracle on the oracle's own replay of the list."""

    def __init__(self, orc, ell, nc, tables, seed):
        self.ell, self.tables = ell, tables
        self.crs = orc.generate_crs_points(ell)
        rng = orc.rng(seed)
        R = rng.g1_affine(nc)
        S = orc.g1_scale(R, rng.fr(nc))
        self.cand = _wire(orc, R, S)
        aff_R, aff_S = _chunks(R, 96), _chunks(S, 96)
        self.post, self.proofs, self.vrand, self.vrand12 = [], [], [], []
        for row in tables:
            vec_R, vec_S = b"".join(aff_R[i] for i in row), b"".join(aff_S[i] for i in row)
            perm, k, mb, rand = rng.shuffle(ell), rng.fr(1), rng.fr(4), rng.fr(3 * (ell + 4) + 9)
            vec_T, vec_U, M = orc.shuffle_permute_and_commit_input(ell, self.crs, vec_R, vec_S, perm, k, mb)
            self.proofs.append(orc.g1_compress_jac(M) + orc.prove(ell, self.crs, vec_R, vec_S, vec_T, vec_U, M, perm, k, mb, rand))
            self.post.append(b"".join(_wire(orc, vec_T, vec_U)))
            self.vrand.append(rng.fr(8))
            self.vrand12.append(rng.fr(12))
            for j, i in enumerate(row):
                aff_R[i], aff_S[i] = vec_T[96 * j:96 * (j + 1)], vec_U[96 * j:96 * (j + 1)]
        self.final, self.pres = replay_bytes(self.cand, tables, self.post)
        assert self.final == _wire(orc, b"".join(aff_R), b"".join(aff_S))     # the byte replay and the oracle's points agree

    def oracle_verdicts(self, orc, cand, post, proofs):
        pres = replay_bytes(cand, self.tables, post)[1]
        return [orc.is_valid_whisk_shuffle_proof(self.ell, self.crs, pres[b], post[b], proofs[b], self.vrand[b]) for b in range(len(self.tables))], pres


@pytest.fixture(scope="module")
def run(orc):
    rnd = random.Random(20262)
    r = Run(orc, ELL, NC, [rnd.sample(range(NC), ELL) for _ in range(NI)], 20262)
    first_write = {}
    for b, row in enumerate(r.tables):
        for i in row:
            first_write.setdefault(i, b)
    from_list = sum(1 for b, row in enumerate(r.tables) for i in row if first_write[i] == b)
    assert from_list <= NC and NI * ELL - from_list > 300                       # nearly every read hits an earlier write
    return r


@pytest.fixture(scope="module")
def mutated(run, orc):
    """(post, proofs, the oracle's verdicts on the as-if pre lists, those pre lists)"""
    from tests import decoding_ref as dr
    post, proofs = list(run.post), list(run.proofs)
    proofs[5] = run.proofs[6]                                                                  # another item's proof
    post[7] = post[7][:96 * (ELL - 1)] + _bad_point(orc) + post[7][96 * (ELL - 1) + 48:]             # an undecodable post tracker
    outside = dr.compress(dr.non_member_points(orc, 1)[0])
    assert dr.decode(outside, orc)[0] == dr.NOT_IN_SUBGROUP
    post[9] = outside + post[9][48:]                                                           # a post tracker outside the subgroup
    post[3] = post[3][96:192] + post[3][:96] + post[3][192:]                                   # two post trackers swapped
    proofs[12] = bytes([proofs[12][0] & 0x7f]) + proofs[12][1:]                                # M without its compression flag
    want, pres = run.oracle_verdicts(orc, run.cand, post, proofs)
    assert want[:3] == [1, 1, 1] and want[3] == 0 and set(want) == {1, 0, -1}
    assert [want[b] for b in (5, 7, 9, 12)] == [0, -1, -1, -1]
    # later items that read what a mutated item wrote are judged on it: items reading the swapped pair fail, one reading the undecodable tracker errs
    swapped = set(run.tables[3][:2])
    assert any(want[b] == 0 and swapped & set(run.tables[b]) for b in (4, 6))
    assert any(want[b] == -1 for b in (8, 10, 11, 13) if run.tables[7][ELL - 1] in run.tables[b] or run.tables[9][0] in run.tables[b])
    return post, proofs, want, pres


def _context(run, **options):
    import curdleproofs_amd as cpx
    c = cpx.Context(0, options=options)
    c.set_crs(run.ell, run.crs)
    return c


@pytest.fixture()
def ctx(run):
    from curdleproofs_amd import whisk
    c = _context(run)
    assert whisk.load_candidate_trackers(c, _trackers(b"".join(run.cand))) == [0] * NC
    yield c
    c.close()


def _answers(results):
    from curdleproofs_amd import whisk
    out = []
    for r in results:
        assert r is True or r is False or isinstance(r, whisk.SerializationError), r
        out.append(1 if r is True else 0 if r is False else -1)
    return out


def _list(c):
    from curdleproofs_amd import whisk
    return [t.to_bytes() for t in whisk.candidate_trackers(c)]


def _posts(post):
    return [_trackers(p) for p in post]


# ---- 1. the honest run ----
def test_honest_run_is_accepted_and_applied(ctx, run, orc):
    from curdleproofs_amd import whisk
    assert ctx._L.cpx_whisk_candidates_size(ctx._h) == NC and _list(ctx) == run.cand          # verbatim
    res, n_applied = whisk.verify_whisk_shuffle_run(ctx, run.tables, _posts(run.post), run.proofs, run.vrand)
    assert res == [True] * NI and n_applied == NI and ctx.batch == NI
    assert _list(ctx) == run.final                                                            # the Python replay, byte for byte
    assert [t.to_bytes() for t in whisk.candidate_trackers(ctx, 3, 5)] == run.final[3:8]
    want, _ = run.oracle_verdicts(orc, run.cand, run.post, run.proofs)
    assert want == [1] * NI                                                                   # the oracle accepts every item on the replayed pre lists
    # the list survives a new CRS and a batch load of another call
    ctx.set_crs(run.ell, run.crs)
    assert whisk.are_valid_whisk_shuffle_proofs(ctx, [_trackers(run.pres[0])], _posts(run.post[:1]), run.proofs[:1], run.vrand[:1]) == [True]
    assert _list(ctx) == run.final
    # ... and a second run goes on from it: the last item again, on the list as item 13 left it, is a proof over other pre trackers
    res, n_applied = whisk.verify_whisk_shuffle_run(ctx, run.tables[-1:], _posts(run.post[-1:]), run.proofs[-1:], run.vrand[-1:])
    pre = b"".join(run.final[i] for i in run.tables[-1])
    assert _answers(res) == [orc.is_valid_whisk_shuffle_proof(ELL, run.crs, pre, run.post[-1], run.proofs[-1], run.vrand[-1])] == [0] and n_applied == 0
    assert _list(ctx) == run.final


# ---- 2. the mutated run ----
def test_mutated_run_matches_the_oracle_and_the_explicit_call(ctx, run, mutated):
    from curdleproofs_amd import whisk
    post, proofs, want, pres = mutated
    res, n_applied = whisk.verify_whisk_shuffle_run(ctx, run.tables, _posts(post), proofs, run.vrand)
    got = _answers(res)
    assert got == want, [(b, g, w) for b, (g, w) in enumerate(zip(got, want)) if g != w]
    first_bad = want.index(0)
    assert n_applied == first_bad == 3
    assert _list(ctx) == replay_bytes(run.cand, run.tables, post, upto=first_bad)[0]           # the replay of that prefix only
    explicit = whisk.are_valid_whisk_shuffle_proofs(ctx, [_trackers(p) for p in pres], _posts(post), proofs, run.vrand)
    assert _answers(explicit) == got


# ---- 3. an undecodable candidate ----
def test_undecodable_candidate_fails_the_items_that_read_it(run, orc):
    from curdleproofs_amd import whisk
    from tests import decoding_ref as dr
    bad = next(i for i in run.tables[1] if i not in run.tables[0])                             # item 1 reads it from the list, item 0 does not
    cand = list(run.cand)
    cand[bad] = cand[bad][:48] + _bad_point(orc)
    c = _context(run)
    try:
        status = whisk.load_candidate_trackers(c, b"".join(cand))
        assert status == [dr.MALFORMED if i == bad else 0 for i in range(NC)]
        assert _list(c) == cand                                                                # kept exactly as given
        res, n_applied = whisk.verify_whisk_shuffle_run(c, run.tables[:3], _posts(run.post[:3]), run.proofs[:3], run.vrand[:3])
        want = run.oracle_verdicts(orc, cand, run.post, run.proofs)[0][:3]
        assert _answers(res) == want and want[:2] == [1, -1] and n_applied == 1
        assert _list(c) == replay_bytes(cand, run.tables, run.post, upto=1)[0]
    finally:
        c.close()


# ---- 4. an index twice inside an item ----
def test_repeated_index_reads_twice_and_the_higher_slot_wins(orc):
    from curdleproofs_amd import whisk
    rnd = random.Random(7)
    a = 11
    others = [i for i in range(NC) if i != a]
    first = [a, a] + rnd.sample(others, ELL - 2)
    second = rnd.sample(others, ELL - 1) + [a]
    r = Run(orc, ELL, NC, [first, second], 4)
    assert r.pres[0][:96] == r.pres[0][96:192] == r.cand[a]                                    # the same tracker twice
    assert r.pres[1][-96:] == r.post[0][96:192] != r.post[0][:96]                              # item 1 reads slot 1's write, not slot 0's
    assert run_is_valid(orc, r) == [1, 1]
    c = _context(r)
    try:
        whisk.load_candidate_trackers(c, b"".join(r.cand))
        res, n_applied = whisk.verify_whisk_shuffle_run(c, r.tables[:1], _posts(r.post[:1]), r.proofs[:1], r.vrand[:1])
        assert res == [True] and n_applied == 1
        assert whisk.candidate_trackers(c, a, 1)[0].to_bytes() == r.post[0][96:192]            # the write-back order
        whisk.load_candidate_trackers(c, b"".join(r.cand))
        res, n_applied = whisk.verify_whisk_shuffle_run(c, r.tables, _posts(r.post), r.proofs, r.vrand)
        assert res == [True, True] and n_applied == 2 and _list(c) == r.final
    finally:
        c.close()


def run_is_valid(orc, r):
    return r.oracle_verdicts(orc, r.cand, r.post, r.proofs)[0]


# ---- 5. the dry run ----
def test_dry_run_gives_the_verdicts_and_leaves_the_list(ctx, run, mutated):
    from curdleproofs_amd import whisk
    post, proofs, want, _ = mutated
    res, n_applied = whisk.verify_whisk_shuffle_run(ctx, run.tables, _posts(post), proofs, run.vrand, apply=False)
    assert _answers(res) == want and n_applied is None and _list(ctx) == run.cand
    res, n_applied = whisk.verify_whisk_shuffle_run(ctx, run.tables, _posts(run.post), run.proofs, run.vrand, apply=False)
    assert res == [True] * NI and n_applied is None and _list(ctx) == run.cand
    res, n_applied, _ = whisk.verify_whisk_shuffle_run(ctx, run.tables, _posts(run.post), run.proofs, run.vrand12, grouped=True, apply=False)
    assert res == [True] * NI and n_applied is None and _list(ctx) == run.cand


# ---- 6. the grouped form ----
def test_grouped_form_gives_the_same_verdicts(ctx, run, mutated, orc):
    from curdleproofs_amd import whisk
    proofs = list(run.proofs)
    proofs[5] = run.proofs[6]                                                                  # one bad item
    want = run.oracle_verdicts(orc, run.cand, run.post, proofs)[0]
    assert want == [0 if b == 5 else 1 for b in range(NI)]
    ctx.set_option("locate_groups_max", 4)               # 14 items: groups of four (a group of one is its own verdict, nothing to recheck)
    res, n_applied, n_rechecked = whisk.verify_whisk_shuffle_run(ctx, run.tables, _posts(run.post), proofs, run.vrand12, grouped=True)
    assert _answers(res) == want and n_applied == 5 and n_rechecked > 0
    assert _list(ctx) == replay_bytes(run.cand, run.tables, run.post, upto=5)[0]
    whisk.load_candidate_trackers(ctx, b"".join(run.cand))
    post, mproofs, mwant, _ = mutated
    res, n_applied, n_rechecked = whisk.verify_whisk_shuffle_run(ctx, run.tables, _posts(post), mproofs, run.vrand12, grouped=True)
    assert _answers(res) == mwant and n_applied == 3 and n_rechecked > 0
    whisk.load_candidate_trackers(ctx, b"".join(run.cand))
    res, n_applied, n_rechecked = whisk.verify_whisk_shuffle_run(ctx, run.tables, _posts(run.post), run.proofs, run.vrand12, grouped=True)
    assert res == [True] * NI and n_applied == NI and n_rechecked == 0 and _list(ctx) == run.final


# ---- 7. refusals ----
def test_refusals_leave_the_list_and_the_verdicts_alone(ctx, run):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    L, h = ctx._L, ctx._h
    count = 3
    tables = [list(r) for r in run.tables[:count]]
    tables[2][ELL - 1] = NC                                                                    # an index equal to the length of the list
    idx = (ctypes.c_uint32 * (count * ELL))(*[i for r in tables for i in r])
    post, proofs, rand = cpx._in(b"".join(run.post[:count])), cpx._in(b"".join(run.proofs[:count])), cpx._in(b"".join(run.vrand[:count]))
    verdict = (ctypes.c_int * count)(*([77] * count))
    applied = ctypes.c_size_t(9)
    assert L.cpx_whisk_verify_shuffle_run(h, count, idx, post, proofs, rand, verdict, ctypes.byref(applied)) == cpx.CPX_ERR_ARG
    assert list(verdict) == [cpx.CPX_ERR_INTERNAL] * count and applied.value == 0              # the pre-fill, nothing else
    assert _list(ctx) == run.cand
    with pytest.raises(cpx.CpxError) as e:
        whisk.verify_whisk_shuffle_run(ctx, tables, _posts(run.post[:count]), run.proofs[:count], run.vrand[:count], grouped=False)
    assert e.value.code == cpx.CPX_ERR_ARG and _list(ctx) == run.cand
    # count = 0 is a no-op; NULL pointers with count > 0 are refused and nothing is written
    verdict[0] = 55
    assert L.cpx_whisk_verify_shuffle_run(h, 0, None, None, None, None, None, None) == cpx.CPX_OK
    assert L.cpx_whisk_verify_shuffle_run(h, 1, None, None, None, None, verdict, None) == cpx.CPX_ERR_ARG and verdict[0] == 55
    # a range outside the list
    for first, n in ((0, NC + 1), (NC, 1), (NC + 1, 0), (1 << 62, 1 << 62)):
        assert L.cpx_whisk_candidates_read(h, first, n, cpx._out(96)) == cpx.CPX_ERR_ARG, (first, n)
    assert L.cpx_whisk_candidates_read(h, NC, 0, None) == cpx.CPX_OK
    # a strict_infinity value other than the one the list was loaded under
    ctx.set_option("strict_infinity", 1)
    with pytest.raises(cpx.CpxError) as e:
        whisk.verify_whisk_shuffle_run(ctx, run.tables[:1], _posts(run.post[:1]), run.proofs[:1], run.vrand[:1])
    assert e.value.code == cpx.CPX_ERR_STATE and _list(ctx) == run.cand
    ctx.set_option("strict_infinity", 0)
    assert whisk.verify_whisk_shuffle_run(ctx, run.tables[:1], _posts(run.post[:1]), run.proofs[:1], run.vrand[:1]) == ([True], 1)
    # dropping the list, and a context that never had one
    assert whisk.load_candidate_trackers(ctx, []) == [] and ctx._L.cpx_whisk_candidates_size(h) == 0
    fresh = _context(run)
    try:
        for c in (ctx, fresh):
            with pytest.raises(cpx.CpxError) as e:
                whisk.verify_whisk_shuffle_run(c, run.tables[:1], _posts(run.post[:1]), run.proofs[:1], run.vrand[:1])
            assert e.value.code == cpx.CPX_ERR_STATE
    finally:
        fresh.close()
    nocrs = cpx.Context(0)
    try:
        whisk.load_candidate_trackers(nocrs, b"".join(run.cand))                               # the list needs no CRS, the run does
        assert nocrs._L.cpx_whisk_verify_shuffle_run(nocrs._h, 1, idx, post, proofs, rand, verdict, None) == cpx.CPX_ERR_STATE
    finally:
        nocrs.close()


# ---- 8. the decoder's work ----
def test_run_call_decodes_the_post_side_only(ctx, run):
    """an identity, not a timing: the explicit call decodes 4 ell + 1 encodings per item before the verifier, the run call 2 ell + 1"""
    from curdleproofs_amd import whisk
    whisk.verify_whisk_shuffle_run(ctx, run.tables[:1], _posts(run.post[:1]), run.proofs[:1], run.vrand[:1], apply=False)      # (decodes the generator)
    ctx.set_profiling(True)
    ctx.reset_stats()
    assert whisk.are_valid_whisk_shuffle_proofs(ctx, [_trackers(p) for p in run.pres], _posts(run.post), run.proofs, run.vrand) == [True] * NI
    explicit = ctx.stat("k_decompress")["units"]
    assert ctx.stat("k_run_gather")["launches"] == 0
    ctx.reset_stats()
    assert whisk.verify_whisk_shuffle_run(ctx, run.tables, _posts(run.post), run.proofs, run.vrand) == ([True] * NI, NI)
    assert explicit - ctx.stat("k_decompress")["units"] == 2 * NI * ELL
    gather, commit = ctx.stat("k_run_gather"), ctx.stat("k_run_commit")
    assert gather["launches"] == 1 and gather["units"] == NI * ELL and gather["alg_bytes"] == NI * ELL * (4 * 96 + 4 + 4)
    touched = len({i for r in run.tables for i in r})
    assert commit["launches"] == 1 and commit["units"] == touched and commit["alg_bytes"] == touched * (4 * 96 + 4 + 8)
    assert ctx.stat("k_shuffle_status")["launches"] == 1
    ctx.set_profiling(False)


# ---- 9. the Whisk shape once ----
def test_whisk_shape_ell_124(orc):
    from curdleproofs_amd import whisk
    ell, nc = 124, 256
    rnd = random.Random(124)
    first = rnd.sample(range(nc), ell)
    second = rnd.sample(first, 60) + rnd.sample([i for i in range(nc) if i not in first], ell - 60)      # reads what the first wrote, and the list
    third = rnd.sample(range(nc), ell)
    r = Run(orc, ell, nc, [first, second, third], 124)
    assert run_is_valid(orc, r) == [1, 1, 1]
    c = _context(r)
    try:
        assert whisk.load_candidate_trackers(c, b"".join(r.cand)) == [0] * nc
        res, n_applied = whisk.verify_whisk_shuffle_run(c, r.tables, _posts(r.post), r.proofs, r.vrand)
        assert res == [True] * 3 and n_applied == 3 and c.batch == 3
        assert _list(c) == r.final
    finally:
        c.close()
