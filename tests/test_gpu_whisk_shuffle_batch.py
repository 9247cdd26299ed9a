"""GPU parity of the batched shuffle calls (cpx_batch_shuffle, cpx_whisk_generate_shuffle_proofs, cpx_whisk_verify_shuffle_proofs and
their Python mirrors).  Expected bytes and verdicts come from the oracle and from the reference's committed vector
whisk_kat["whisk_shuffle_proof_ell124"], never from the library under test.  ell = 28 (n = 32) is the smallest size the suite uses; the
reference vector needs ell = 124.  Counts 1, 3, 9 and 12 put count * ell = 28 .. 336 elements on both sides of the 64-lane and 256-lane
group sizes of the new kernels, with dead lanes in the last group."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

R_ = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
ELL = 28
N = ELL + 4
NI = 12
BAD_POINT = bytes([0x80]) + bytes(46) + b"\x05"     # compressed, x = 5: not the x of a curve point
MUTATIONS = ("untouched", "two post trackers swapped", "pre and post exchanged", "another item's proof", "M and A swapped", "undecodable tracker in pre",
             "undecodable tracker in post", "M without the compression flag", "last scalar 0xff..ff", "tracker outside the subgroup",
             "M a non-canonical infinity", "untouched")
NONCANONICAL = MUTATIONS.index("M a non-canonical infinity")


def _cat(ts):
    return b"".join(t.to_bytes() for t in ts)


def _trackers(blob):
    from curdleproofs_amd import whisk
    return [whisk.WhiskTracker(blob[96 * j:96 * j + 48], blob[96 * j + 48:96 * j + 96]) for j in range(len(blob) // 96)]


def _zip_compress(orc, vec_a, vec_b):
    ca, cb = orc.g1_compress(vec_a), orc.g1_compress(vec_b)
    return b"".join(ca[48 * j:48 * (j + 1)] + cb[48 * j:48 * (j + 1)] for j in range(len(ca) // 48))


def _item(orc, ell, crs, rng, k=None, perm=None):
    """one shuffle with its witness and draws, and everything the oracle makes of it"""
    vec_R = rng.g1_affine(ell)
    vec_S = orc.g1_scale(vec_R, rng.fr(ell))
    it = dict(vec_R=vec_R, vec_S=vec_S, perm=rng.shuffle(ell) if perm is None else perm, k=rng.fr(1) if k is None else k, mb=rng.fr(4),
              rand=rng.fr(3 * (ell + 4) + 9), vrand=rng.fr(8))
    return _finish(orc, ell, crs, it)


def _finish(orc, ell, crs, it):
    it["vec_T"], it["vec_U"], it["M"] = orc.shuffle_permute_and_commit_input(ell, crs, it["vec_R"], it["vec_S"], it["perm"], it["k"], it["mb"])
    it["pre"] = _zip_compress(orc, it["vec_R"], it["vec_S"])
    it["post"] = _zip_compress(orc, it["vec_T"], it["vec_U"])
    it["proof"] = orc.g1_compress_jac(it["M"]) + orc.prove(ell, crs, it["vec_R"], it["vec_S"], it["vec_T"], it["vec_U"], it["M"], it["perm"], it["k"], it["mb"],
                                                          it["rand"])
    return it


class Data:
    """12 shuffles at ell = 28 with the oracle's results, and the verifier's mutated batch with the oracle's answers"""

    def __init__(self, orc):
        from tests import decoding_ref as dr
        fr = lambda v: orc.fr_from_canonical_bytes((v % R_).to_bytes(32, "little"))
        self.crs = orc.generate_crs_points(ELL)
        rng = orc.rng(20261)
        # item 0: k = 1 and the identity permutation; item 1: k = r - 1 and the reversal
        special = {0: dict(k=fr(1), perm=list(range(ELL))), 1: dict(k=fr(R_ - 1), perm=list(range(ELL - 1, -1, -1)))}
        self.items = [_item(orc, ELL, self.crs, rng, **special.get(i, {})) for i in range(NI)]
        # ---- the verifier's batch: item j mutated as MUTATIONS[j] says ----
        pre, post, proofs = ([it[key] for it in self.items] for key in ("pre", "post", "proof"))
        m = MUTATIONS.index
        j = m("two post trackers swapped")
        post[j] = post[j][96:192] + post[j][:96] + post[j][192:]
        j = m("pre and post exchanged")
        pre[j], post[j] = post[j], pre[j]
        j = m("another item's proof")
        proofs[j] = self.items[j + 1]["proof"]
        j = m("M and A swapped")
        proofs[j] = proofs[j][48:96] + proofs[j][:48] + proofs[j][96:]
        j = m("undecodable tracker in pre")
        pre[j] = pre[j][:96 * 5 + 48] + BAD_POINT + pre[j][96 * 6:]
        j = m("undecodable tracker in post")
        post[j] = post[j][:96 * (ELL - 1)] + BAD_POINT + post[j][96 * (ELL - 1) + 48:]
        j = m("M without the compression flag")
        proofs[j] = bytes([proofs[j][0] & 0x7f]) + proofs[j][1:]
        j = m("last scalar 0xff..ff")
        proofs[j] = proofs[j][:-32] + b"\xff" * 32
        j = m("tracker outside the subgroup")
        outside = dr.compress(dr.non_member_points(orc, 1)[0])
        assert dr.decode(outside, orc)[0] == dr.NOT_IN_SUBGROUP
        post[j] = outside + post[j][48:]
        proofs[NONCANONICAL] = bytes([0xc0]) + bytes(46) + b"\x01" + proofs[NONCANONICAL][48:]
        self.vpre, self.vpost, self.vproofs = pre, post, proofs
        self.vrand = [it["vrand"] for it in self.items]
        self.want = {}
        for strict in (False, True):
            orc.set_strict_infinity(strict)
            try:
                self.want[strict] = [orc.is_valid_whisk_shuffle_proof(ELL, self.crs, pre[j], post[j], proofs[j], self.vrand[j]) for j in range(NI)]
            finally:
                orc.set_strict_infinity(False)
        # every kind of answer is present, and the two settings differ exactly at the non-canonical item
        assert set(self.want[False]) == {1, 0, -1}
        assert self.want[False][0] == 1 and self.want[False][NI - 1] == 1
        assert [a != b for a, b in zip(self.want[False], self.want[True])] == [j == NONCANONICAL for j in range(NI)]
        assert self.want[True][NONCANONICAL] == -1

    def args(self, count):
        it = self.items[:count]
        return dict(permutations=[x["perm"] for x in it], ks=[x["k"] for x in it], vec_m_blinders=[x["mb"] for x in it], rands=[x["rand"] for x in it])


@pytest.fixture(scope="module")
def data(orc):
    return Data(orc)


def _context(data, **options):
    import curdleproofs_amd as cpx
    c = cpx.Context(0, options=options)
    c.set_crs(ELL, data.crs)
    return c


@pytest.fixture(scope="module")
def ctx(data):
    c = _context(data)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev_ctx(data):
    """every batch runs the device-resident protocol (the `device_resident` variant of test_engine_variants_stay_bit_exact)"""
    c = _context(data, device_min_batch=1)
    yield c
    c.close()


def _answers(results):
    from curdleproofs_amd import whisk
    out = []
    for r in results:
        assert r is True or r is False or isinstance(r, whisk.SerializationError), r
        out.append(1 if r is True else 0 if r is False else -1)
    return out


# ---- 1. the shuffle step ----
@pytest.mark.parametrize("count", [1, 3, 9])
def test_shuffle_step_matches_the_oracle(ctx, data, orc, count):
    from curdleproofs_amd import util
    it = data.items[:count]
    call = lambda c: util.shuffle_permute_and_commit_inputs(c, [x["vec_R"] for x in it], [x["vec_S"] for x in it], [x["perm"] for x in it], [x["k"] for x in it],
                                                            [x["mb"] for x in it])
    got = call(ctx)
    assert ctx.batch == count
    assert len(got) == count
    for i, (t, u, m) in enumerate(got):
        assert t == it[i]["vec_T"] and u == it[i]["vec_U"], "item %d of %d" % (i, count)
        assert orc.g1_compress_jac(m) == orc.g1_compress_jac(it[i]["M"]), "M of item %d of %d" % (i, count)
    assert got[0][0] == it[0]["vec_R"]                               # k = 1 and the identity permutation: T = R
    for options in ({"fix_bits": 8}, {"fix_bits": 16}, {"scale_any_point": 1}):
        c = _context(data, **options)
        try:
            if "fix_bits" in options:
                assert c.get_option("fix_bits_effective") == options["fix_bits"]
            other = call(c)
        finally:
            c.close()
        assert [(t, u, orc.g1_compress_jac(m)) for t, u, m in other] == [(t, u, orc.g1_compress_jac(m)) for t, u, m in got], options


# ---- 2. the prover against the reference's vector ----
def test_prover_matches_the_reference_vector_at_ell_124(orc, whisk_kat):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    ell = 124
    crs = orc.generate_crs_points(ell)                 # CurdleproofsCrs::generate_crs(ELL)
    rng = orc.rng(0)                                   # whisk.rs:416-424: per tracker k = Fr::rand, r = Fr::rand
    gen = orc.g1_generator()
    kr = [(rng.fr(1), rng.fr(1)) for _ in range(ell)]
    vec_R = orc.g1_scale(gen * ell, b"".join(r for _, r in kr))
    vec_S = orc.g1_scale(vec_R, b"".join(k for k, _ in kr))
    first = dict(vec_R=vec_R, vec_S=vec_S, perm=rng.shuffle(ell), k=rng.fr(1), mb=rng.fr(4), rand=rng.fr(3 * (ell + 4) + 9), vrand=rng.fr(8))
    items = [_finish(orc, ell, crs, first), _item(orc, ell, crs, orc.rng(77))]
    c = cpx.Context(0)
    try:
        c.set_crs(ell, crs)
        got = whisk.generate_whisk_shuffle_proofs(c, [_trackers(x["pre"]) for x in items], [x["perm"] for x in items], [x["k"] for x in items],
                                                  [x["mb"] for x in items], [x["rand"] for x in items])
        assert c.batch == 2
        assert got[0][1] == bytes.fromhex(whisk_kat["whisk_shuffle_proof_ell124"])     # whisk.rs:455, byte for byte
        for i, x in enumerate(items):
            assert got[i][1] == x["proof"] and len(got[i][1]) == 4496, i
            assert _cat(got[i][0]) == x["post"], i
        res = whisk.are_valid_whisk_shuffle_proofs(c, [_trackers(x["pre"]) for x in items], [_trackers(x["post"]) for x in items], [x["proof"] for x in items],
                                                   [x["vrand"] for x in items])
        assert res == [True, True]
        assert [orc.is_valid_whisk_shuffle_proof(ell, crs, x["pre"], x["post"], x["proof"], x["vrand"]) for x in items] == [1, 1]
    finally:
        c.close()


# ---- 3. the prover on both engine paths ----
@pytest.mark.parametrize("path", ["host_driven", "device_resident"])
def test_prover_matches_the_oracle_on_both_engine_paths(ctx, dev_ctx, data, path):
    from curdleproofs_amd import whisk
    c, count = (ctx, 3) if path == "host_driven" else (dev_ctx, 5)
    pre = [_trackers(x["pre"]) for x in data.items[:count]]
    got = whisk.generate_whisk_shuffle_proofs(c, pre, **data.args(count))
    assert c.batch == count
    for i in range(count):
        assert got[i][1] == data.items[i]["proof"], "proof %d (%s)" % (i, path)
        assert _cat(got[i][0]) == data.items[i]["post"], "post trackers %d (%s)" % (i, path)
    # one undecodable tracker in the middle item: that item is the reference's Err, every other item is unchanged
    bad = count // 2
    pre[bad] = pre[bad][:7] + [whisk.WhiskTracker(BAD_POINT, pre[bad][7].k_r_G)] + pre[bad][8:]
    again = whisk.generate_whisk_shuffle_proofs(c, pre, **data.args(count))
    assert again[bad] is None
    assert [again[i] == got[i] for i in range(count)] == [i != bad for i in range(count)]


def test_prover_status_and_zero_bytes_for_an_undecodable_tracker(ctx, data):
    """the C-ABI level: status = CPX_ERR_DESERIALIZE and zero bytes for that item only"""
    import curdleproofs_amd as cpx
    count, bad = 3, 1
    rec = 48 + ctx.proof_size
    pre = [x["pre"] for x in data.items[:count]]
    pre[bad] = pre[bad][:96 * 3] + BAD_POINT + pre[bad][96 * 3 + 48:]
    post = (ctypes.c_uint8 * (96 * ELL * count))(*([0xaa] * (96 * ELL * count)))
    proofs = (ctypes.c_uint8 * (rec * count))(*([0xaa] * (rec * count)))
    st = (ctypes.c_int * count)(*([77] * count))
    a = data.args(count)
    perm = (ctypes.c_uint32 * (count * ELL))(*[x for p in a["permutations"] for x in p])
    rc = ctx._L.cpx_whisk_generate_shuffle_proofs(ctx._h, count, cpx._in(b"".join(pre)), perm, cpx._in(b"".join(a["ks"])), cpx._in(b"".join(a["vec_m_blinders"])),
                                                  cpx._in(b"".join(a["rands"])), post, proofs, st)
    assert rc == cpx.CPX_OK
    assert list(st) == [cpx.CPX_ERR_DESERIALIZE if i == bad else cpx.CPX_OK for i in range(count)]
    pb, fb = bytes(post), bytes(proofs)
    assert pb[96 * ELL * bad:96 * ELL * (bad + 1)] == bytes(96 * ELL) and fb[rec * bad:rec * (bad + 1)] == bytes(rec)
    for i in (0, 2):
        assert pb[96 * ELL * i:96 * ELL * (i + 1)] == data.items[i]["post"] and fb[rec * i:rec * (i + 1)] == data.items[i]["proof"]


# ---- 4. the verifier ----
@pytest.mark.parametrize("strict", [0, 1], ids=["ark_0_4_infinity", "strict_infinity"])
@pytest.mark.parametrize("path", ["host_driven", "device_resident"])
def test_verifier_matches_the_oracle_on_every_mutation(data, path, strict):
    from curdleproofs_amd import whisk
    options = {"strict_infinity": strict}
    if path == "device_resident":
        options["device_min_batch"] = 1
    c = _context(data, **options)
    try:
        got = _answers(whisk.are_valid_whisk_shuffle_proofs(c, [_trackers(p) for p in data.vpre], [_trackers(p) for p in data.vpost], data.vproofs, data.vrand))
        assert c.batch == NI
    finally:
        c.close()
    want = data.want[bool(strict)]
    assert got == want, [(MUTATIONS[j], g, w) for j, (g, w) in enumerate(zip(got, want)) if g != w]


# ---- 5. the batch equals the single calls ----
def test_batch_agrees_with_the_single_calls(ctx, data):
    from curdleproofs_amd import whisk
    pre, post = [_trackers(p) for p in data.vpre], [_trackers(p) for p in data.vpost]
    batch = whisk.are_valid_whisk_shuffle_proofs(ctx, pre, post, data.vproofs, data.vrand)
    for j in range(NI):
        try:
            one = whisk.is_valid_whisk_shuffle_proof(ctx, pre[j], post[j], data.vproofs[j], rand=data.vrand[j])
        except whisk.SerializationError as e:
            one = e
        assert _answers([one]) == _answers([batch[j]]), MUTATIONS[j]
    count, bad = 4, 2
    pre = [_trackers(x["pre"]) for x in data.items[:count]]
    pre[bad] = pre[bad][:-1] + [whisk.WhiskTracker(pre[bad][-1].r_G, BAD_POINT)]
    a = data.args(count)
    made = whisk.generate_whisk_shuffle_proofs(ctx, pre, **a)
    for j in range(count):
        try:
            one = whisk.generate_whisk_shuffle_proof(ctx, pre[j], permutation=a["permutations"][j], k=a["ks"][j], vec_m_blinders=a["vec_m_blinders"][j],
                                                     rand=a["rands"][j])
        except whisk.SerializationError:
            one = None
        assert one == made[j], j
    assert made[bad] is None and made[0] is not None


# ---- 6. launch counts ----
def test_launch_count_does_not_depend_on_the_count(data):
    """profiling on: the kernels around the batch prover / verifier are launched as often for 3 items as for 9, the new ones once per call"""
    from curdleproofs_amd import util, whisk
    new = ("k_shuffle_status", "k_shuffle_gather", "k_shuffle_commit")
    names = ("k_decompress", "k_smul", "k_compress") + new
    c = _context(data)
    try:
        whisk.are_valid_whisk_shuffle_proofs(c, [_trackers(data.vpre[0])], [_trackers(data.vpost[0])], data.vproofs[:1], data.vrand[:1])   # (decodes the generator)
        c.set_profiling(True)
        seen = {}
        for count in (3, 9):
            it = data.items[:count]
            pre, post = [_trackers(x["pre"]) for x in it], [_trackers(x["post"]) for x in it]
            stats = []
            c.reset_stats()
            util.shuffle_permute_and_commit_inputs(c, [x["vec_R"] for x in it], [x["vec_S"] for x in it], [x["perm"] for x in it], [x["k"] for x in it],
                                                   [x["mb"] for x in it])
            stats.append({k: c.stat(k)["launches"] for k in names})
            c.reset_stats()
            whisk.generate_whisk_shuffle_proofs(c, pre, **data.args(count))
            stats.append({k: c.stat(k)["launches"] for k in names})
            c.reset_stats()
            assert whisk.are_valid_whisk_shuffle_proofs(c, pre, post, [x["proof"] for x in it], [x["vrand"] for x in it]) == [True] * count
            stats.append({k: c.stat(k)["launches"] for k in names})
            seen[count] = stats
        assert seen[3] == seen[9]
        step, prove, verify = seen[3]
        assert {k: step[k] for k in names} == dict(k_decompress=0, k_smul=1, k_compress=0, k_shuffle_status=1, k_shuffle_gather=1, k_shuffle_commit=1)
        assert {k: prove[k] for k in new} == dict(k_shuffle_status=1, k_shuffle_gather=1, k_shuffle_commit=1)
        assert {k: verify[k] for k in new} == dict(k_shuffle_status=1, k_shuffle_gather=0, k_shuffle_commit=0)
    finally:
        c.close()


# ---- 7. state ----
def test_loaded_batch_crs_and_argument_errors(data, orc):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    count = 3
    it = data.items[:count]
    pre = [_trackers(x["pre"]) for x in it]
    pre[1] = [whisk.WhiskTracker(BAD_POINT, pre[1][0].k_r_G)] + pre[1][1:]
    c = _context(data)
    try:
        got = whisk.generate_whisk_shuffle_proofs(c, pre, **data.args(count))
        assert c.batch == count and got[1] is None
        # the loaded instances are the call's: the returned proofs (M stripped) verify on them; the placeholder of the bad item is not judged
        verdicts = c.verify_batch([(g[1][48:] if g else bytes(c.proof_size)) for g in got], b"".join(x["vrand"] for x in it))
        assert [verdicts[i] for i in (0, 2)] == [cpx.CPX_OK] * 2
        assert c.crs_sums() == orc.crs_sums(ELL, data.crs)
        # a row that is no permutation: CPX_ERR_ARG before anything is launched, and the loaded batch still verifies
        a = data.args(count)
        a["permutations"] = [a["permutations"][0], [0] * ELL, a["permutations"][2]]
        with pytest.raises(cpx.CpxError) as e:
            whisk.generate_whisk_shuffle_proofs(c, pre, **a)
        assert e.value.code == cpx.CPX_ERR_ARG
        with pytest.raises(cpx.CpxError) as e:
            c.shuffle_batch(b"".join(x["vec_R"] for x in it), b"".join(x["vec_S"] for x in it), [x for p in a["permutations"] for x in p],
                            b"".join(x["k"] for x in it), b"".join(x["mb"] for x in it))
        assert e.value.code == cpx.CPX_ERR_ARG
        assert c.batch == count
        again = c.verify_batch([(g[1][48:] if g else bytes(c.proof_size)) for g in got], b"".join(x["vrand"] for x in it))
        assert again == verdicts
        res = whisk.are_valid_whisk_shuffle_proofs(c, [_trackers(x["pre"]) for x in it], [_trackers(x["post"]) for x in it], [x["proof"] for x in it],
                                                   [x["vrand"] for x in it])
        assert res == [True] * count and c.batch == count
        assert c.verify_batch([x["proof"][48:] for x in it], b"".join(x["vrand"] for x in it)) == [cpx.CPX_OK] * count
        # count = 0 is a no-op, NULL pointers with count > 0 are refused and nothing is written
        st = (ctypes.c_int * 1)(55)
        assert c._L.cpx_whisk_verify_shuffle_proofs(c._h, 0, None, None, None, None, None) == cpx.CPX_OK
        assert c._L.cpx_whisk_generate_shuffle_proofs(c._h, 0, None, None, None, None, None, None, None, None) == cpx.CPX_OK
        assert c._L.cpx_batch_shuffle(c._h, 0, None, None, None, None, None, None, None, None) == cpx.CPX_OK
        assert c._L.cpx_whisk_verify_shuffle_proofs(c._h, 1, None, None, None, None, st) == cpx.CPX_ERR_ARG and st[0] == 55
        assert c.batch == count
    finally:
        c.close()
    fresh = cpx.Context(0)                                       # no CRS
    try:
        buf = (ctypes.c_uint8 * 8192)()
        st = (ctypes.c_int * 1)(55)
        perm = (ctypes.c_uint32 * ELL)(*range(ELL))
        assert fresh._L.cpx_whisk_verify_shuffle_proofs(fresh._h, 1, buf, buf, buf, buf, st) == cpx.CPX_ERR_STATE
        assert fresh._L.cpx_whisk_generate_shuffle_proofs(fresh._h, 1, buf, perm, buf, buf, buf, buf, buf, st) == cpx.CPX_ERR_STATE
        assert fresh._L.cpx_batch_shuffle(fresh._h, 1, buf, buf, perm, buf, buf, buf, buf, buf) == cpx.CPX_ERR_STATE
        assert fresh.batch == 0
    finally:
        fresh.close()
