"""Group elements drawn on the device (k_rng_g1_scan / _sqrt / _select and k_clear_cofactor behind cpx_rng_g1, cpx_rng_instance_draws,
cpx_crs_generate and cpx_g1_clear_cofactor) against the oracle's `G1Projective::rand` and the integer model (tests/stdrng_g1_ref.py, pinned to
the oracle without a GPU by tests/test_rng_g1_check_cpu.py, which also states what the cases of tests/rng_g1_cases.py cover), and against the
reference's own committed vector: whisk.rs:416-456 and the README example come out of the number 0 with nothing made by the oracle."""
import ctypes
import os

import pytest

from tests import rng_g1_cases as gc
from tests import stdrng_g1_ref as g1
from tests import stdrng_ref as sr
from tests.stdrng_ref import StdRng

pytestmark = pytest.mark.gpu

FILL = bytes([0x5a])


def _buf(b):
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


@pytest.fixture(scope="module")
def cpx():
    import curdleproofs_amd
    return curdleproofs_amd


@pytest.fixture(scope="module")
def plain(cpx):
    c = cpx.Context(0)          # no CRS: cpx_rng_g1 and cpx_g1_clear_cofactor need none
    yield c
    c.close()


def test_device_build_of_rng_g1_check(tmp_path):
    """the pieces of G1::rand on the device, bit for bit against the host twin and the model"""
    from curdleproofs_amd import build
    assert os.path.exists(build.check_path("rng_g1_check")), "curdleproofs_amd/_lib/rng_g1_check is missing: build() makes it"
    assert gc.list_operations(build.check_path("rng_g1_check")) == gc.TABLE
    records = gc.check_records()
    dev = gc.run_check(build.check_path("rng_g1_check"), records, tmp_path, "dev")
    twin = gc.run_check(gc.build_host_twin(tmp_path), records, tmp_path, "twin")
    total = sum(len(r) for _, r in records)
    assert gc.assert_rows(records, dev, twin, ("device", "host twin")) == total
    assert gc.assert_rows(records, dev, gc.check_expected(), ("device", "model")) == total


def _draw(ctx, cpx, streams, n_each, round_cap, compressed=True):
    """cpx_rng_g1 on the streams under the option; returns (affine, compressed, states, rounds)"""
    count = len(streams)
    ctx.set_option("rng_g1_round_cap", round_cap)
    try:
        st = _buf(b"".join(gc.state_of(d) for d in streams))
        aff, comp = _buf(FILL * (96 * n_each * count)), _buf(FILL * (48 * n_each * count))
        assert ctx._L.cpx_rng_g1(ctx._h, count, st, n_each, aff, comp if compressed else None) == cpx.CPX_OK
        return bytes(aff), bytes(comp), bytes(st), ctx.get_option("rng_g1_last_rounds")
    finally:
        ctx.set_option("rng_g1_round_cap", 0)


def _check(ctx, cpx, orc, streams, n_each, round_cap):
    want = [gc.expected(orc, d, n_each) for d in streams]
    aff, comp, st, rounds = _draw(ctx, cpx, streams, n_each, round_cap)
    for i, w in enumerate(want):
        assert aff[96 * n_each * i: 96 * n_each * (i + 1)] == w[0], "stream %d: points" % i
        assert comp[48 * n_each * i: 48 * n_each * (i + 1)] == w[1], "stream %d: encodings" % i
        assert st[40 * i: 40 * (i + 1)] == w[2], "stream %d: state" % i
    # the returned states CONTINUE: the next Fr::rand from them is the oracle's / the model's
    stb, out = _buf(st), (ctypes.c_uint8 * (32 * len(streams)))()
    assert ctx._L.cpx_rng_fr(ctx._h, len(streams), stb, 1, out) == cpx.CPX_OK
    assert bytes(out) == b"".join(w[3] for w in want)
    assert ctx.batch == 0
    return rounds


_CASES = gc.g1_cases()
_IDS = ["%dx%d" % (c, n) for c, n in gc.SHAPES] + ["searched/" + name.replace(" ", "_") for name in sorted(gc.searched())]


@pytest.mark.parametrize("case", range(len(_CASES)), ids=_IDS)
def test_rng_g1(plain, cpx, orc, case):
    streams, n_each, round_cap = _CASES[case]
    rounds = _check(plain, cpx, orc, streams, n_each, round_cap)
    name = _IDS[case]
    if name == "searched/last":
        assert rounds == 1          # the last candidate of round one supplied the last point
    elif name == "searched/first":
        assert rounds == 2          # ... the first candidate of round two
    elif round_cap == 0:
        assert rounds == 1          # (the default cap: more than one round is a 5-sigma accident, and none of these streams has it)


_LATER = [(s, n, c) for s, n, _ in _CASES if n <= 8 for c in gc.CAPS] + [(gc.shape_streams(1), 65, 64)]


@pytest.mark.parametrize("case", range(len(_LATER)), ids=["%dx%d/cap=%d" % (len(s), n, c) for s, n, c in _LATER])
def test_later_rounds_give_the_same_bytes(plain, cpx, orc, case):
    streams, n_each, round_cap = _LATER[case]
    rounds = _check(plain, cpx, orc, streams, n_each, round_cap)
    if round_cap < n_each:          # (fewer candidates than points owed: one round cannot do)
        assert rounds > 1


@pytest.mark.parametrize("ell", [4, 28, 124])
def test_crs_generate(cpx, orc, ell):
    want = orc.generate_crs_points(ell)
    c, ref = cpx.Context(0), cpx.Context(0)
    try:
        st, pts = _buf(StdRng.seed_from_u64(0).state()), _buf(FILL * (96 * (ell + 7)))
        assert c._L.cpx_crs_generate(c._h, ell, st, pts) == cpx.CPX_OK
        assert bytes(pts) == want
        ref.set_crs(ell, want)
        g, h = _buf(bytes(96)), _buf(bytes(96))
        assert c._L.cpx_crs_sums(c._h, g, h) == cpx.CPX_OK and (bytes(g), bytes(h)) == ref.crs_sums()
        assert c._L.cpx_proof_size(c._h) == ref.proof_size
        _, pos = gc.walk(("seed", 0, 0), ell + 7)
        after = StdRng(sr.key_from_u64(0), pos)
        behind = after.state()
        assert bytes(st) == behind
        out = (ctypes.c_uint8 * 32)()
        assert c._L.cpx_rng_fr(c._h, 1, st, 1, out) == cpx.CPX_OK and bytes(out) == after.fr(1)
        # points_out may be NULL; the Python wrapper leaves the context as set_crs does
        from curdleproofs_amd import crs
        assert crs.generate_crs(ref, ell) == want and (ref.ell, ref.n, ref.crs_points) == (ell, ell + 4, want)
        st2 = _buf(StdRng.seed_from_u64(0).state())
        assert c._L.cpx_crs_generate(c._h, ell, st2, None) == cpx.CPX_OK and bytes(st2) == behind
    finally:
        c.close()
        ref.close()


@pytest.mark.parametrize("options", [{}, {"device_min_batch": 1}], ids=["host-driven", "device-resident"])
def test_reference_kat_with_nothing_from_the_oracle(cpx, whisk_kat, options):
    """whisk.rs:416-456 from the number 0 on the product API alone: generate_crs(124), 124 trackers from (k, r) draws, one shuffle proof"""
    from curdleproofs_amd import crs, whisk
    from curdleproofs_amd.rng import StdRng as Rng
    ell = 124
    kat = bytes.fromhex(whisk_kat["whisk_shuffle_proof_ell124"])
    c = cpx.Context(0, options=options)
    try:
        crs.generate_crs(c, ell)                                  # crs.rs:63: its own StdRng::seed_from_u64(0)
        rng = Rng.seed_from_u64(0)
        kr = rng.fr(c, 2 * ell)
        pre, _ = whisk.trackers_from_k_r(c, [kr[64 * i:64 * i + 32] for i in range(ell)], [kr[64 * i + 32:64 * i + 64] for i in range(ell)])
        post, proof = whisk.generate_whisk_shuffle_proof(c, pre, rng=rng)
        assert len(kat) == 4496 and proof == kat                  # whisk.rs:455
        assert whisk.is_valid_whisk_shuffle_proof(c, pre, post, proof, rand=rng.fr(c, 8))
    finally:
        c.close()


@pytest.mark.parametrize("count", [1, 3])
def test_readme_example_from_the_number_zero(cpx, orc, count):
    """README.md:76-118 for StdRng(seed), seed = 0 .. count - 1, on the C-ABI: cpx_crs_generate -> cpx_rng_instance_draws -> cpx_rng_fr(4) ->
    cpx_batch_shuffle -> cpx_batch_prove_rng -> cpx_rng_fr(8) -> cpx_batch_verify, against orc.make_instance"""
    ell, n = 28, 32
    c = cpx.Context(0)
    try:
        L, h = c._L, c._h
        st0, crs_pts = _buf(StdRng.seed_from_u64(0).state()), _buf(bytes(96 * (ell + 7)))
        assert L.cpx_crs_generate(h, ell, st0, crs_pts) == cpx.CPX_OK
        want = [orc.make_instance(ell, seed, bytes(crs_pts)) for seed in range(count)]
        st = _buf(b"".join(StdRng.seed_from_u64(seed).state() for seed in range(count)))
        perm, k = (ctypes.c_uint32 * (count * ell))(), _buf(bytes(32 * count))
        R, S = _buf(bytes(96 * ell * count)), _buf(bytes(96 * ell * count))
        assert L.cpx_rng_instance_draws(h, count, st, perm, k, R, S) == cpx.CPX_OK
        assert [list(perm[ell * i: ell * (i + 1)]) for i in range(count)] == [w["permutation"] for w in want]
        assert bytes(k) == b"".join(w["k"] for w in want)
        assert bytes(R) == b"".join(w["vec_R"] for w in want) and bytes(S) == b"".join(w["vec_S"] for w in want)
        mb = _buf(bytes(128 * count))
        assert L.cpx_rng_fr(h, count, st, 4, mb) == cpx.CPX_OK and bytes(mb) == b"".join(w["vec_m_blinders"] for w in want)
        T, U, M = _buf(bytes(96 * ell * count)), _buf(bytes(96 * ell * count)), _buf(bytes(144 * count))
        assert L.cpx_batch_shuffle(h, count, R, S, perm, k, mb, T, U, M) == cpx.CPX_OK
        assert bytes(T) == b"".join(w["vec_T"] for w in want) and bytes(U) == b"".join(w["vec_U"] for w in want)
        assert c.normalize(bytes(M)) == c.normalize(b"".join(w["M"] for w in want))
        psz = L.cpx_proof_size(h)
        proofs = _buf(bytes(psz * count))
        assert L.cpx_batch_prove_rng(h, perm, k, mb, st, proofs) == cpx.CPX_OK
        assert [bytes(proofs)[psz * i: psz * (i + 1)] for i in range(count)] == [w["proof"] for w in want]
        vr = _buf(bytes(256 * count))
        assert L.cpx_rng_fr(h, count, st, 8, vr) == cpx.CPX_OK and bytes(vr) == b"".join(w["verifier_rand"] for w in want)
        verdict = (ctypes.c_int * count)(*([cpx.CPX_ERR_INTERNAL] * count))
        assert L.cpx_batch_verify(h, proofs, vr, verdict) == cpx.CPX_OK and list(verdict) == [cpx.CPX_OK] * count
        # the Python wrapper draws the same set; any output may be NULL and the states advance all the same
        from curdleproofs_amd import crs, rng as prng
        assert crs.generate_crs(c, ell) == bytes(crs_pts)           # (the wrapper's own load: it is what tells the Python object its ell)
        rngs =[prng.StdRng.seed_from_u64(seed) for seed in range(count)]
        draws = prng.instance_draws(c, rngs)
        assert [(d[0], d[1], d[2], d[3]) for d in draws] == [(w["permutation"], w["k"], w["vec_R"], w["vec_S"]) for w in want]
        st2 = _buf(b"".join(StdRng.seed_from_u64(seed).state() for seed in range(count)))
        assert L.cpx_rng_instance_draws(h, count, st2, None, None, None, None) == cpx.CPX_OK
        assert bytes(st2) == b"".join(r.state for r in rngs)
    finally:
        c.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_clear_cofactor(plain, cpx, orc, n):
    """the clear_cofactor rows through the C-ABI, n points a call (the work-group inversion's edges), against the model; on subgroup points
    also against cpx_g1_scale by h"""
    t = gc.torsion_points()
    names = sorted(t)
    pts = [t[names[(i + n) % len(names)]] for i in range(n)]
    got = plain.clear_cofactor(b"".join(g1.to_wire(p) for p in pts))
    want = {name: g1.to_wire(g1.clear_cofactor(t[name])) for name in names}
    assert got == b"".join(want[names[(i + n) % len(names)]] for i in range(n))
    sub = [t[name] for name in names if name.startswith("subgroup")]
    sub = (sub * n)[:n]
    wire = b"".join(g1.to_wire(p) for p in sub)
    h_wire = (g1.H * pow(2, 256, sr.R) % sr.R).to_bytes(32, "little")        # the cofactor as a Montgomery scalar
    assert plain.clear_cofactor(wire) == plain.scale(wire, h_wire)


def test_argument_errors_write_nothing(plain, cpx, orc):
    L, h = plain._L, plain._h
    good = StdRng.seed_from_u64(4)
    late = StdRng(good.key, sr.POS_LIMIT).state()
    # cpx_rng_g1: NULLs, a state at the position limit in slot 2 of 3, limits exceeded by one; count = 0 and n_each = 0 are no-ops
    states = good.state() + late + StdRng(good.key, 7).state()
    st, aff, comp = _buf(states), _buf(FILL * (96 * 2 * 3)), _buf(FILL * (48 * 2 * 3))
    assert L.cpx_rng_g1(h, 3, st, 2, aff, comp) == cpx.CPX_ERR_ARG
    assert L.cpx_rng_g1(h, 3, None, 2, aff, comp) == cpx.CPX_ERR_ARG and L.cpx_rng_g1(h, 3, st, 2, None, comp) == cpx.CPX_ERR_ARG
    assert L.cpx_rng_g1(h, (1 << 20) + 1, st, 1, aff, None) == cpx.CPX_ERR_ARG and L.cpx_rng_g1(h, 1, st, (1 << 16) + 1, aff, None) == cpx.CPX_ERR_ARG
    assert L.cpx_rng_g1(h, (1 << 11) + 1, st, 1 << 11, aff, None) == cpx.CPX_ERR_ARG            # count * n_each = 2^22 + 2^11
    assert L.cpx_rng_g1(h, 0, None, 2, None, None) == cpx.CPX_OK and L.cpx_rng_g1(h, 3, st, 0, aff, comp) == cpx.CPX_OK
    assert bytes(st) == states and bytes(aff) == FILL * len(aff) and bytes(comp) == FILL * len(comp)
    # cpx_g1_clear_cofactor
    assert L.cpx_g1_clear_cofactor(h, None, 1, aff) == cpx.CPX_ERR_ARG and L.cpx_g1_clear_cofactor(h, aff, 1, None) == cpx.CPX_ERR_ARG
    assert L.cpx_g1_clear_cofactor(h, aff, (1 << 24) + 1, aff) == cpx.CPX_ERR_ARG and L.cpx_g1_clear_cofactor(h, None, 0, None) == cpx.CPX_OK
    assert bytes(aff) == FILL * len(aff)
    # cpx_rng_instance_draws: no CRS is a state error
    st = _buf(good.state())
    assert L.cpx_rng_instance_draws(h, 1, st, None, None, None, None) == cpx.CPX_ERR_STATE and bytes(st) == good.state()
    # cpx_crs_generate at ell = 27 refuses as cpx_ctx_set_crs does, before a word is drawn; a late state and NULL are argument errors
    c = cpx.Context(0)
    try:
        st, pts = _buf(good.state()), _buf(FILL * (96 * 34))
        assert L.cpx_crs_generate(c._h, 27, st, pts) == cpx.CPX_ERR_NOT_POW2 == L.cpx_ctx_set_crs(c._h, 27, _buf(orc.generate_crs_points(28)), 35)
        assert L.cpx_crs_generate(c._h, 0, st, pts) == cpx.CPX_ERR_NOT_POW2
        assert L.cpx_crs_generate(c._h, 28, None, pts) == cpx.CPX_ERR_ARG
        assert bytes(st) == good.state() and bytes(pts) == FILL * len(pts) and L.cpx_proof_size(c._h) == 0
        st = _buf(late)
        assert L.cpx_crs_generate(c._h, 28, st, pts) == cpx.CPX_ERR_ARG and bytes(st) == late and bytes(pts) == FILL * len(pts)
        # with a CRS: a late state among the instance streams writes nothing
        st = _buf(good.state())
        assert L.cpx_crs_generate(c._h, 4, st, None) == cpx.CPX_OK
        states = good.state() + late + StdRng(good.key, 7).state()
        st, perm, k = _buf(states), (ctypes.c_uint32 * 12)(*([77] * 12)), _buf(FILL * 96)
        R, S = _buf(FILL * (96 * 4 * 3)), _buf(FILL * (96 * 4 * 3))
        assert L.cpx_rng_instance_draws(c._h, 3, st, perm, k, R, S) == cpx.CPX_ERR_ARG
        assert L.cpx_rng_instance_draws(c._h, 3, None, perm, k, R, S) == cpx.CPX_ERR_ARG
        assert L.cpx_rng_instance_draws(c._h, 0, None, None, None, None, None) == cpx.CPX_OK
        assert bytes(st) == states and list(perm) == [77] * 12 and bytes(k) == FILL * 96 and bytes(R) == FILL * len(R) and bytes(S) == FILL * len(S)
    finally:
        c.close()
