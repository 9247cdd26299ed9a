"""GPU parity of the multiples of the generator made on its fixed-base table (Context.generator_mul, whisk.trackers_from_k_r,
whisk.k_commitments -> cpx_g1_generator_mul / cpx_whisk_trackers_from_k_r).  Expected bytes come from the oracle — g1_scale on
g1_generator(), g1_compress, fr_mul — never from the library under test; the scalar sets are tests/gen_mul_cases.py, whose coverage of the
table tests/test_generator_mul_cpu.py asserts.  Counts 1, 2, 63, 64, 65 and 257 put one wave, the wave boundary and several work-groups
behind one call; a tracker call runs 2 or 3 lanes per pair."""
import ctypes

import pytest

from tests import gen_mul_cases as gc

pytestmark = pytest.mark.gpu

FR, AFF = 32, 96
COUNTS = (0, 1, 2, 63, 64, 65, 257)
PAIR_COUNTS = (1, 65, 257)
IDENTITY = bytes([0xc0]) + bytes(47)
K_ZERO, R_ZERO, BOTH_ONE, PRODUCT_ONE, PRODUCT_MINUS_ONE = 0, 1, 2, 3, 4      # positions of the edge pairs


@pytest.fixture(scope="module")
def ctx():
    import curdleproofs_amd as cpx
    c = cpx.Context(0)
    yield c
    c.close()


def _wire(orc, ints):
    return orc.fr_from_canonical_bytes(gc.to_bytes(ints))


def _multiples(orc, wire):
    """(affine, compressed) of wire[i] * G from the oracle"""
    n = len(wire) // FR
    aff = orc.g1_scale(orc.g1_generator() * n, wire) if n else b""
    return aff, orc.g1_compress(aff) if n else b""


class Pairs:
    """257 (k, r) pairs — five edge pairs, then seeded random ones — and what the oracle and the single calls make of them"""

    def __init__(self, orc, ctx):
        from curdleproofs_amd import whisk
        n = max(PAIR_COUNTS)
        rnd = orc.fr_to_canonical_bytes(orc.rng(20261017).fr(2 * n))
        val = [int.from_bytes(rnd[FR * i:FR * (i + 1)], "little") for i in range(2 * n)]
        k, r = val[:n], val[n:]
        k[K_ZERO] = 0
        r[R_ZERO] = 0
        k[BOTH_ONE] = r[BOTH_ONE] = 1
        r[PRODUCT_ONE] = pow(k[PRODUCT_ONE], -1, gc.R_)
        r[PRODUCT_MINUS_ONE] = gc.R_ - pow(k[PRODUCT_MINUS_ONE], -1, gc.R_)
        assert k[PRODUCT_ONE] * r[PRODUCT_ONE] % gc.R_ == 1 and k[PRODUCT_MINUS_ONE] * r[PRODUCT_MINUS_ONE] % gc.R_ == gc.R_ - 1
        kw, rw = _wire(orc, k), _wire(orc, r)
        self.k = [kw[FR * i:FR * (i + 1)] for i in range(n)]
        self.r = [rw[FR * i:FR * (i + 1)] for i in range(n)]
        # the reference's definition (whisk.rs:45-55): r G, then k (r G) by a scalar multiplication of THAT point
        r_g = orc.g1_scale(orc.g1_generator() * n, rw)
        k_r_g = orc.g1_scale(r_g, kw)
        cr, ckr = orc.g1_compress(r_g), orc.g1_compress(k_r_g)
        self.trackers = [whisk.WhiskTracker(cr[48 * i:48 * (i + 1)], ckr[48 * i:48 * (i + 1)]) for i in range(n)]
        ck = _multiples(orc, kw)[1]
        self.commitments = [ck[48 * i:48 * (i + 1)] for i in range(n)]
        # ... and the shortcut's: (k r) G with the oracle's Fr product
        assert orc.g1_compress(orc.g1_scale(orc.g1_generator() * n, orc.fr_mul(kw, rw))) == ckr
        assert self.trackers[K_ZERO].k_r_G == IDENTITY and self.commitments[K_ZERO] == IDENTITY
        assert self.trackers[R_ZERO].r_G == IDENTITY and self.trackers[R_ZERO].k_r_G == IDENTITY
        gen = orc.g1_compress(orc.g1_generator())
        assert self.trackers[BOTH_ONE].to_bytes() == gen * 2 and self.trackers[PRODUCT_ONE].k_r_G == gen
        # the library's single calls on the same pairs, once for all counts
        self.single = [whisk.WhiskTracker.from_k_r(ctx, self.k[i], self.r[i]) for i in range(n)]
        k_g = whisk.bls_g1_scalar_multiply(ctx, whisk.g1_generator(ctx) * n, kw)
        self.single_commitments = [whisk.to_bytes_g1affine(ctx, k_g[AFF * i:AFF * (i + 1)]) for i in range(n)]


@pytest.fixture(scope="module")
def pairs(orc, ctx):
    return Pairs(orc, ctx)


@pytest.mark.parametrize("count", COUNTS)
def test_generator_mul_matches_the_oracle(ctx, orc, count):
    wire = orc.rng(1000 + count).fr(count) if count else b""
    want_aff, want_comp = _multiples(orc, wire)
    aff, comp = ctx.generator_mul(wire, compressed=True)
    assert len(aff) == AFF * count and len(comp) == 48 * count
    assert aff == want_aff and comp == want_comp
    assert ctx.generator_mul(wire) == want_aff


def test_coverage_set_in_one_call(ctx, orc):
    """every (half, window, digit magnitude, sign) the table can be asked for (asserted on the CPU: test_generator_mul_cpu.py)"""
    scalars = gc.coverage_scalars()
    wire = _wire(orc, scalars)
    want_aff, want_comp = _multiples(orc, wire)
    aff, comp = ctx.generator_mul(wire, compressed=True)
    for i, k in enumerate(scalars):
        assert comp[48 * i:48 * (i + 1)] == want_comp[48 * i:48 * (i + 1)], hex(k)
    assert aff == want_aff


def test_edge_scalars(ctx, orc):
    scalars = gc.edge_scalars()
    wire = _wire(orc, scalars)
    want_aff, want_comp = _multiples(orc, wire)
    aff, comp = ctx.generator_mul(wire, compressed=True)
    for i, k in enumerate(scalars):
        assert comp[48 * i:48 * (i + 1)] == want_comp[48 * i:48 * (i + 1)], hex(k)
        assert aff[AFF * i:AFF * (i + 1)] == want_aff[AFF * i:AFF * (i + 1)], hex(k)
    assert scalars[0] == 0 and aff[:AFF] == bytes(AFF) and comp[:48] == IDENTITY          # the zero scalar: the identity in both encodings
    assert comp[48:96] == orc.g1_compress(orc.g1_generator())


@pytest.mark.parametrize("count", PAIR_COUNTS)
def test_trackers_from_k_r_match_the_two_step_definition(ctx, pairs, count):
    from curdleproofs_amd import whisk
    trackers, commitments = whisk.trackers_from_k_r(ctx, pairs.k[:count], pairs.r[:count])
    assert len(trackers) == count and len(commitments) == count
    for i in range(count):
        assert trackers[i] == pairs.trackers[i], "tracker %d of %d" % (i, count)
        assert commitments[i] == pairs.commitments[i], "commitment %d of %d" % (i, count)
        assert trackers[i] == pairs.single[i] and commitments[i] == pairs.single_commitments[i]      # WhiskTracker.from_k_r, bls_g1_scalar_multiply(G, k)
    assert whisk.k_commitments(ctx, pairs.k[:count]) == pairs.commitments[:count]


def test_proofs_over_the_new_trackers_verify(ctx, pairs, orc):
    from curdleproofs_amd import whisk
    count = 65
    trackers, commitments = whisk.trackers_from_k_r(ctx, pairs.k[:count], pairs.r[:count])
    bl = orc.rng(77).fr(count)
    proofs = whisk.generate_whisk_tracker_proofs(ctx, trackers, pairs.k[:count], [bl[FR * i:FR * (i + 1)] for i in range(count)])
    assert all(p is not None for p in proofs)
    assert whisk.are_valid_whisk_tracker_proofs(ctx, trackers, commitments, proofs) == [True] * count
    # and the oracle accepts them for the oracle's own trackers and commitments
    for i in (0, 1, 2, 3, 4, 64):
        assert orc.is_valid_whisk_tracker_proof(pairs.trackers[i].to_bytes(), pairs.commitments[i], proofs[i]) == 1


def test_output_and_argument_conventions(ctx, pairs, orc):
    import curdleproofs_amd as cpx
    L, h = ctx._L, ctx._h
    n = 5
    kw, rw = b"".join(pairs.k[:n]), b"".join(pairs.r[:n])
    want_trk = b"".join(t.to_bytes() for t in pairs.trackers[:n])
    want_kc = b"".join(pairs.commitments[:n])
    want_aff, want_comp = _multiples(orc, kw)
    fill = lambda size: (ctypes.c_uint8 * size)(*([0xaa] * size))
    # either output may be NULL
    a, c = fill(AFF * n), fill(48 * n)
    assert L.cpx_g1_generator_mul(h, n, cpx._in(kw), a, None) == cpx.CPX_OK and bytes(a) == want_aff
    assert L.cpx_g1_generator_mul(h, n, cpx._in(kw), None, c) == cpx.CPX_OK and bytes(c) == want_comp
    assert L.cpx_g1_generator_mul(h, n, cpx._in(kw), None, None) == cpx.CPX_OK
    t, c = fill(96 * n), fill(48 * n)
    assert L.cpx_whisk_trackers_from_k_r(h, n, cpx._in(kw), cpx._in(rw), t, None) == cpx.CPX_OK and bytes(t) == want_trk
    assert L.cpx_whisk_trackers_from_k_r(h, n, cpx._in(kw), cpx._in(rw), None, c) == cpx.CPX_OK and bytes(c) == want_kc
    assert L.cpx_whisk_trackers_from_k_r(h, n, cpx._in(kw), cpx._in(rw), None, None) == cpx.CPX_OK
    # count = 0 is a no-op, a NULL input with count > 0 is CPX_ERR_ARG and nothing is written
    t, c = fill(96), fill(48)
    assert L.cpx_g1_generator_mul(h, 0, None, None, None) == cpx.CPX_OK
    assert L.cpx_whisk_trackers_from_k_r(h, 0, None, None, t, c) == cpx.CPX_OK
    assert L.cpx_g1_generator_mul(h, 1, None, t, c) == cpx.CPX_ERR_ARG
    assert L.cpx_whisk_trackers_from_k_r(h, 1, None, cpx._in(rw), t, c) == cpx.CPX_ERR_ARG
    assert L.cpx_whisk_trackers_from_k_r(h, 1, cpx._in(kw), None, t, c) == cpx.CPX_ERR_ARG
    assert L.cpx_g1_generator_mul(h, (1 << 23) + 1, cpx._in(kw), t, c) == cpx.CPX_ERR_ARG          # more than 2^23 items: refused before anything is read
    assert bytes(t) == b"\xaa" * 96 and bytes(c) == b"\xaa" * 48
    # limbs that are not a reduced field element stand for limbs / 2^256 mod r, as the k of the batched tracker prover: w + r gives what w gives
    w = int.from_bytes(pairs.k[5], "little")
    assert w + gc.R_ < 1 << 256
    big = (w + gc.R_).to_bytes(32, "little")
    assert ctx.generator_mul(big, compressed=True)[1] == pairs.commitments[5]
    c = fill(48)
    t = fill(96)
    assert L.cpx_whisk_trackers_from_k_r(h, 1, cpx._in(big), cpx._in(pairs.r[5]), t, c) == cpx.CPX_OK
    assert bytes(t) == pairs.trackers[5].to_bytes() and bytes(c) == pairs.commitments[5]


def test_loaded_batch_is_left_alone_and_a_second_context_agrees(pairs, orc):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    ell = 28
    crs = orc.generate_crs_points(ell)
    inst = orc.make_instance(ell, 0, crs)
    n = 9
    c = cpx.Context(0)
    try:
        c.set_crs(ell, crs)
        c.load_batch(*(inst[k] * 2 for k in ("vec_R", "vec_S", "vec_T", "vec_U", "M")))
        before = c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2)
        assert c.batch == 2 and before == [cpx.CPX_OK] * 2
        assert whisk.trackers_from_k_r(c, pairs.k[:n], pairs.r[:n]) == (pairs.trackers[:n], pairs.commitments[:n])
        assert whisk.k_commitments(c, pairs.k[:n]) == pairs.commitments[:n]
        assert c.batch == 2
        assert c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2) == before
    finally:
        c.close()
    fresh = cpx.Context(0)                                       # no CRS, nothing loaded, a table of its own
    try:
        assert whisk.trackers_from_k_r(fresh, pairs.k[:n], pairs.r[:n]) == (pairs.trackers[:n], pairs.commitments[:n])
        assert fresh.batch == 0
    finally:
        fresh.close()


def test_launch_count_does_not_depend_on_the_count(pairs):
    """profiling on: one k_gen_mul and one k_compress per call for 1 pair as for 257, and the table is built once per context"""
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    names = ("k_gen_table", "k_gen_mul", "k_compress", "k_smul", "k_finalize", "k_decompress")
    c = cpx.Context(0)
    try:
        c.set_profiling(True)
        whisk.k_commitments(c, pairs.k[:1])                      # the context's first call decodes the generator and builds the table
        assert c.stat("k_gen_table")["launches"] == 1 and c.stat("k_gen_mul")["launches"] == 1
        seen = {}
        for count in (1, 257):
            c.reset_stats()
            whisk.trackers_from_k_r(c, pairs.k[:count], pairs.r[:count])
            t = {k: c.stat(k)["launches"] for k in names}
            c.reset_stats()
            whisk.k_commitments(c, pairs.k[:count])
            seen[count] = (t, {k: c.stat(k)["launches"] for k in names})
        assert seen[1] == seen[257]
        assert seen[1][0] == {"k_gen_table": 0, "k_gen_mul": 1, "k_compress": 1, "k_smul": 0, "k_finalize": 0, "k_decompress": 0}
        assert seen[1][1] == seen[1][0]
        assert c.stat("k_gen_mul")["units"] == 257
    finally:
        c.close()
