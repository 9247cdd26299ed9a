"""GPU parity of the batched tracker-proof calls (curdleproofs_amd.whisk.generate_whisk_tracker_proofs / are_valid_whisk_tracker_proofs
-> cpx_whisk_generate_tracker_proofs / cpx_whisk_verify_tracker_proofs).  Expected bytes and verdicts come from the oracle and from the
reference's committed vector whisk_kat["tracker_proof"], never from the library under test.  Sizes: 1, 8, 9 and 37 proofs put 2 count
relations, 3 count scalar multiplications and 5 count points on both sides of the 16-quads-per-wave boundary with dead quads in the last wave."""
import pytest

pytestmark = pytest.mark.gpu

R_ = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
N = 37
COUNTS = (1, 8, 9, 37)
BAD_POINT = bytes([0x80]) + bytes(46) + b"\x05"     # compressed, x = 5: not the x of a curve point
IDENTITY = bytes([0xc0]) + bytes(47)
# items with edge-case witnesses (item 0 carries the draws of the reference's own test, whisk.rs:381-402)
K_ZERO, K_ONE, K_MINUS_ONE, BLINDER_ZERO, R_ONE = 1, 2, 3, 5, 6
# verifier batch: the item at each of these positions is mutated, in the order of MUTATIONS
MUTATED = range(8, 17)
MUTATIONS = ("wrong commitment", "tracker halves swapped", "s + 1", "A and B swapped", "s = 0xff..ff", "commitment without the compression flag",
             "x >= p", "curve point outside the subgroup", "non-canonical infinity")


class Data:
    """37 (tracker, k, blinder) triples, the oracle's proofs for them, and the mutated verifier batch — all from the oracle"""

    def __init__(self, orc):
        from curdleproofs_amd import whisk
        from tests import decoding_ref as dr
        fr = lambda v: orc.fr_from_canonical_bytes((v % R_).to_bytes(32, "little"))
        rng0, rng = orc.rng(0), orc.rng(1234)
        self.k, self.r, self.b = [], [], []
        for i in range(N):
            src = rng0 if i == 0 else rng
            k, r, b = src.fr(1), src.fr(1), src.fr(1)      # whisk.rs:383-392: k, then r inside WhiskTracker::from_k, then the blinder
            if i == K_ZERO:
                k = fr(0)
            if i == K_ONE:
                k = fr(1)
            if i == K_MINUS_ONE:
                k = fr(R_ - 1)
            if i == BLINDER_ZERO:
                b = fr(0)
            if i == R_ONE:
                r = fr(1)
            self.k.append(k)
            self.r.append(r)
            self.b.append(b)
        gen = orc.g1_generator()
        r_g = orc.g1_scale(gen * N, b"".join(self.r))
        k_r_g = orc.g1_scale(r_g, b"".join(self.k))
        k_g = orc.g1_scale(gen * N, b"".join(self.k))
        cr, ckr, ck = orc.g1_compress(r_g), orc.g1_compress(k_r_g), orc.g1_compress(k_g)
        cut = lambda blob, i: blob[48 * i:48 * (i + 1)]
        self.trackers = [whisk.WhiskTracker(cut(cr, i), cut(ckr, i)) for i in range(N)]
        self.commitments = [cut(ck, i) for i in range(N)]
        assert self.trackers[R_ONE].r_G == orc.g1_compress(gen) and self.commitments[K_ZERO] == IDENTITY
        self.proofs = [orc.generate_whisk_tracker_proof(self.trackers[i].to_bytes(), self.k[i], self.b[i]) for i in range(N)]
        assert self.proofs[BLINDER_ZERO][:96] == IDENTITY * 2      # blinder = 0: A and B are the identity
        # ---- the verifier's batch ----
        vt, vc, vp = list(self.trackers), list(self.commitments), list(self.proofs)
        m = iter(MUTATED)
        i = next(m)
        vc[i] = self.commitments[i + 10]
        i = next(m)
        vt[i] = whisk.WhiskTracker(vt[i].k_r_G, vt[i].r_G)
        i = next(m)
        vp[i] = vp[i][:96] + ((int.from_bytes(vp[i][96:], "little") + 1) % R_).to_bytes(32, "little")
        i = next(m)
        vp[i] = vp[i][48:96] + vp[i][:48] + vp[i][96:]
        i = next(m)
        vp[i] = vp[i][:96] + b"\xff" * 32
        i = next(m)
        vc[i] = bytes(48)
        i = next(m)
        vp[i] = dr.encode(dr.P + 1, 0x80) + vp[i][48:]
        i = next(m)
        outside = dr.compress(dr.non_member_points(orc, 1)[0])
        assert dr.decode(outside, orc)[0] == dr.NOT_IN_SUBGROUP
        vt[i] = whisk.WhiskTracker(outside, vt[i].k_r_G)
        i = next(m)
        self.noncanonical = i
        vp[i] = bytes([0xc0]) + bytes(46) + b"\x01" + vp[i][48:]
        assert i == MUTATED[-1] and len(MUTATIONS) == len(MUTATED)
        self.vt, self.vc, self.vp = vt, vc, vp
        self.want = {}
        for strict in (False, True):
            orc.set_strict_infinity(strict)
            try:
                self.want[strict] = [orc.is_valid_whisk_tracker_proof(vt[j].to_bytes(), vc[j], vp[j]) for j in range(N)]
            finally:
                orc.set_strict_infinity(False)
        # what the oracle says about the mutations: every kind of answer is present
        w = self.want[False]
        assert [w[j] for j in MUTATED] == [0, 0, 0, 0, -1, -1, -1, -1, 0]
        assert all(w[j] == 1 for j in range(N) if j not in MUTATED)
        assert [a != b for a, b in zip(self.want[False], self.want[True])] == [j == self.noncanonical for j in range(N)]
        assert self.want[True][self.noncanonical] == -1


@pytest.fixture(scope="module")
def data(orc):
    return Data(orc)


@pytest.fixture(scope="module")
def ctx():
    import curdleproofs_amd as cpx
    c = cpx.Context(0)
    yield c
    c.close()


def _answers(results):
    """list of True / False / SerializationError instances -> the oracle's 1 / 0 / -1"""
    from curdleproofs_amd import whisk
    out = []
    for r in results:
        assert r is True or r is False or isinstance(r, whisk.SerializationError), r
        out.append(1 if r is True else 0 if r is False else -1)
    return out


@pytest.mark.parametrize("count", COUNTS)
def test_prover_matches_the_reference_vector_and_the_oracle(ctx, data, whisk_kat, count):
    from curdleproofs_amd import whisk
    trackers = list(data.trackers[:count])
    bad = count // 2 if count >= 8 else None
    if bad is not None:
        assert bad not in (0, K_ZERO, K_ONE, K_MINUS_ONE, BLINDER_ZERO, R_ONE)
        trackers[bad] = whisk.WhiskTracker(BAD_POINT, trackers[bad].k_r_G)
    got = whisk.generate_whisk_tracker_proofs(ctx, trackers, data.k[:count], data.b[:count])
    assert len(got) == count
    assert got[0] == bytes.fromhex(whisk_kat["tracker_proof"])         # whisk.rs:401, byte for byte
    for i in range(count):
        if i == bad:
            assert got[i] is None, "an undecodable tracker is that item's SerializationError"
        else:
            assert got[i] == data.proofs[i], "item %d of %d" % (i, count)


def test_prover_status_and_zero_bytes_for_an_undecodable_tracker(ctx, data):
    """the C-ABI level: status = CPX_ERR_DESERIALIZE and 128 zero bytes for that item only"""
    import ctypes
    import curdleproofs_amd as cpx
    count, bad = 9, 4
    tr = [t.to_bytes() for t in data.trackers[:count]]
    tr[bad] = tr[bad][:48] + BAD_POINT
    out = (ctypes.c_uint8 * (128 * count))(*([0xaa] * (128 * count)))
    st = (ctypes.c_int * count)(*([77] * count))
    rc = ctx._L.cpx_whisk_generate_tracker_proofs(ctx._h, count, cpx._in(b"".join(tr)), cpx._in(b"".join(data.k[:count])), cpx._in(b"".join(data.b[:count])), out, st)
    assert rc == cpx.CPX_OK
    assert list(st) == [cpx.CPX_ERR_DESERIALIZE if i == bad else cpx.CPX_OK for i in range(count)]
    blob = bytes(out)
    assert blob[128 * bad:128 * (bad + 1)] == bytes(128)
    assert all(blob[128 * i:128 * (i + 1)] == data.proofs[i] for i in range(count) if i != bad)


@pytest.mark.parametrize("strict", [0, 1], ids=["ark_0_4_infinity", "strict_infinity"])
def test_verifier_matches_the_oracle_on_all_37(data, strict):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    c = cpx.Context(0, options={"strict_infinity": strict})
    try:
        got = _answers(whisk.are_valid_whisk_tracker_proofs(c, data.vt, data.vc, data.vp))
    finally:
        c.close()
    assert len(got) == N
    assert got == data.want[bool(strict)], [(j, g, w) for j, (g, w) in enumerate(zip(got, data.want[bool(strict)])) if g != w]


@pytest.mark.parametrize("quad_max", [1 << 20, 0], ids=["quad_decoder", "lane_decoder"])
def test_verifier_on_both_decoding_kernels(data, quad_max):
    """5 x 37 = 185 points: option decompress_quad_max on the context puts them on k_decompress_quad or on k_decompress"""
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    c = cpx.Context(0, options={"decompress_quad_max": quad_max})
    try:
        got = _answers(whisk.are_valid_whisk_tracker_proofs(c, data.vt, data.vc, data.vp))
        made = whisk.generate_whisk_tracker_proofs(c, data.trackers, data.k, data.b)
    finally:
        c.close()
    assert got == data.want[False]
    assert made == data.proofs


def test_batch_agrees_with_the_single_calls(ctx, data):
    from curdleproofs_amd import whisk
    batch = whisk.are_valid_whisk_tracker_proofs(ctx, data.vt, data.vc, data.vp)
    for j in range(N):
        try:
            one = whisk.is_valid_whisk_tracker_proof(ctx, data.vt[j], data.vc[j], data.vp[j])
        except whisk.SerializationError as e:
            one = e
        assert _answers([one]) == _answers([batch[j]]), j
    trackers = list(data.trackers)
    trackers[20] = whisk.WhiskTracker(trackers[20].r_G, BAD_POINT)
    made = whisk.generate_whisk_tracker_proofs(ctx, trackers, data.k, data.b)
    for j in range(N):
        try:
            one = whisk.generate_whisk_tracker_proof(ctx, trackers[j], data.k[j], data.b[j])
        except whisk.SerializationError:
            one = None
        assert one == made[j], j
    assert made[20] is None and made[19] == data.proofs[19]


def test_loaded_batch_and_crs_are_left_alone(data, orc):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    ell = 28
    crs = orc.generate_crs_points(ell)
    inst = orc.make_instance(ell, 0, crs)
    c = cpx.Context(0)
    try:
        c.set_crs(ell, crs)
        c.load_batch(*(inst[k] * 2 for k in ("vec_R", "vec_S", "vec_T", "vec_U", "M")))
        before = c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2)
        assert c.batch == 2 and before == [cpx.CPX_OK] * 2
        assert _answers(whisk.are_valid_whisk_tracker_proofs(c, data.vt[:9], data.vc[:9], data.vp[:9])) == data.want[False][:9]
        assert whisk.generate_whisk_tracker_proofs(c, data.trackers[:9], data.k[:9], data.b[:9]) == data.proofs[:9]
        assert c.batch == 2
        assert c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2) == before
        assert c.crs_sums() == orc.crs_sums(ell, crs)
    finally:
        c.close()
    fresh = cpx.Context(0)                                       # no CRS, nothing loaded
    try:
        assert _answers(whisk.are_valid_whisk_tracker_proofs(fresh, data.vt[:3], data.vc[:3], data.vp[:3])) == data.want[False][:3]
        assert whisk.generate_whisk_tracker_proofs(fresh, data.trackers[:3], data.k[:3], data.b[:3]) == data.proofs[:3]
        assert whisk.are_valid_whisk_tracker_proofs(fresh, [], [], []) == [] and whisk.generate_whisk_tracker_proofs(fresh, [], [], []) == []
        import ctypes
        st = (ctypes.c_int * 1)(55)
        assert fresh._L.cpx_whisk_verify_tracker_proofs(fresh._h, 0, None, None, None, None) == cpx.CPX_OK     # count = 0: a no-op
        assert fresh._L.cpx_whisk_generate_tracker_proofs(fresh._h, 0, None, None, None, None, None) == cpx.CPX_OK
        assert fresh._L.cpx_whisk_verify_tracker_proofs(fresh._h, 1, None, None, None, st) == cpx.CPX_ERR_ARG and st[0] == 55
        assert fresh.batch == 0
    finally:
        fresh.close()


def test_launch_count_does_not_depend_on_the_count(data):
    """profiling on: each new kernel is launched as often for 9 proofs as for 37 — once per call, never per item"""
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    c = cpx.Context(0)
    try:
        whisk.are_valid_whisk_tracker_proofs(c, data.vt[:1], data.vc[:1], data.vp[:1])     # (the context's first call decodes the generator)
        c.set_profiling(True)
        seen = {}
        for count in (9, 37):
            c.reset_stats()
            whisk.are_valid_whisk_tracker_proofs(c, data.vt[:count], data.vc[:count], data.vp[:count])
            v = {k: c.stat(k)["launches"] for k in ("k_tracker_challenge", "k_tracker_relations", "k_decompress")}
            c.reset_stats()
            whisk.generate_whisk_tracker_proofs(c, data.trackers[:count], data.k[:count], data.b[:count])
            p = {k: c.stat(k)["launches"] for k in ("k_tracker_challenge", "k_tracker_relations", "k_decompress", "k_smul", "k_compress")}
            seen[count] = (v, p)
        assert seen[9] == seen[37]
        assert seen[9][0] == {"k_tracker_challenge": 1, "k_tracker_relations": 1, "k_decompress": 1}
        assert seen[9][1] == {"k_tracker_challenge": 1, "k_tracker_relations": 0, "k_decompress": 1, "k_smul": 1, "k_compress": 1}
    finally:
        c.close()


# ---- more than one rewritten array in one call ----
# Non-canonical encodings of the infinity (compression and infinity flag set, anything else behind them): three different spellings
NONCANONICAL = (bytes([0xe0]) + bytes(47), bytes([0xc0]) + bytes(46) + b"\x01", b"\xff" * 48)
_ANSWER = {0: 1, -5: -1}      # CPX_OK, CPX_ERR_DESERIALIZE; anything else a rejection


def _oracle_under(orc, strict, ask):
    orc.set_strict_infinity(bool(strict))
    try:
        return ask()
    finally:
        orc.set_strict_infinity(False)


def _codes(verdict):
    import curdleproofs_amd as cpx
    assert cpx.CPX_OK == 0 and cpx.CPX_ERR_DESERIALIZE == -5
    assert all(v in (cpx.CPX_OK, cpx.CPX_ERR_VERIFY, cpx.CPX_ERR_DESERIALIZE) for v in verdict), list(verdict)
    return [_ANSWER.get(v, 0) for v in verdict]


def test_noncanonical_infinities_in_three_arrays_of_one_call(data, orc):
    """item 1's r_G (trackers), item 3's k_commitment and item 5's A (proofs) are non-canonical infinities at once: with strict_infinity = 0
    every one of the three arrays is rewritten in a copy of its own, and all three copies are read by the same call.  Verdicts from the
    oracle under the same setting; the caller's buffers are left as they were."""
    import ctypes
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    count = 8
    vt, vc, vp = list(data.vt[:count]), list(data.vc[:count]), list(data.vp[:count])
    assert all(j not in MUTATED for j in range(count))
    vt[1] = whisk.WhiskTracker(NONCANONICAL[0], vt[1].k_r_G)
    vc[3] = NONCANONICAL[1]
    vp[5] = NONCANONICAL[2] + vp[5][48:]
    want = {s: _oracle_under(orc, s, lambda: [orc.is_valid_whisk_tracker_proof(vt[j].to_bytes(), vc[j], vp[j]) for j in range(count)]) for s in (0, 1)}
    assert [a != b for a, b in zip(want[0], want[1])] == [j in (1, 3, 5) for j in range(count)]
    assert [want[1][j] for j in (1, 3, 5)] == [-1] * 3 and -1 not in want[0]
    tr, kc, pf = b"".join(t.to_bytes() for t in vt), b"".join(vc), b"".join(vp)
    weights = orc.rng(778).fr(2 * count)
    for strict, grouped in ((0, False), (1, False), (0, True)):
        c = cpx.Context(0, options={"strict_infinity": strict, "locate_groups_max": 2})      # grouped: two groups of four items
        try:
            b_tr, b_kc, b_pf = cpx._in(tr), cpx._in(kc), cpx._in(pf)
            verdict = (ctypes.c_int * count)(*([77] * count))
            if grouped:
                rechecked = ctypes.c_size_t(0)
                rc = c._L.cpx_whisk_verify_tracker_proofs_grouped(c._h, count, b_tr, b_kc, b_pf, cpx._in(weights), verdict, ctypes.byref(rechecked))
            else:
                rc = c._L.cpx_whisk_verify_tracker_proofs(c._h, count, b_tr, b_kc, b_pf, verdict)
        finally:
            c.close()
        assert rc == cpx.CPX_OK
        assert _codes(verdict) == want[strict], (strict, grouped, list(verdict))
        assert (bytes(b_tr), bytes(b_kc), bytes(b_pf)) == (tr, kc, pf)


def test_noncanonical_infinities_in_three_arrays_of_one_shuffle_call(orc):
    """the same for the shuffle verifier at ell = 28: item 0 has a pre tracker, item 1 a post tracker and item 2 an M that is a non-canonical
    infinity"""
    import ctypes
    import curdleproofs_amd as cpx
    from tests.test_gpu_whisk_shuffle_batch import ELL, _item
    count = 3
    crs = orc.generate_crs_points(ELL)
    rng = orc.rng(20262)
    items = [_item(orc, ELL, crs, rng) for _ in range(count)]
    pre, post, proofs = ([it[key] for it in items] for key in ("pre", "post", "proof"))
    put = lambda blob, at, enc: blob[:at] + enc + blob[at + 48:]
    pre[0] = put(pre[0], 96 * 3, NONCANONICAL[0])                     # r_G of tracker 3
    post[1] = put(post[1], 96 * (ELL - 1) + 48, NONCANONICAL[1])      # k_r_G of the last tracker
    proofs[2] = put(proofs[2], 0, NONCANONICAL[2])
    vrand = [it["vrand"] for it in items]
    want = {s: _oracle_under(orc, s, lambda: [orc.is_valid_whisk_shuffle_proof(ELL, crs, pre[j], post[j], proofs[j], vrand[j]) for j in range(count)])
            for s in (0, 1)}
    assert want[1] == [-1] * count and -1 not in want[0]
    b = [b"".join(x) for x in (pre, post, proofs)]
    for strict in (0, 1):
        c = cpx.Context(0, options={"strict_infinity": strict})
        try:
            c.set_crs(ELL, crs)
            bufs = [cpx._in(x) for x in b]
            verdict = (ctypes.c_int * count)(*([77] * count))
            rc = c._L.cpx_whisk_verify_shuffle_proofs(c._h, count, bufs[0], bufs[1], bufs[2], cpx._in(b"".join(vrand)), verdict)
        finally:
            c.close()
        assert rc == cpx.CPX_OK
        assert _codes(verdict) == want[strict], (strict, list(verdict))
        assert [bytes(x) for x in bufs] == b
