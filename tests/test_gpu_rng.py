"""The prover's draws made on the device (k_rng_draw behind cpx_rng_fr, cpx_rng_shuffle_draws, cpx_whisk_generate_shuffle_proofs_rng and
cpx_batch_prove_rng) against the Python model of the reference's StdRng (tests/stdrng_ref.py, pinned to the oracle's without a GPU by
tests/test_rng_check_cpu.py) and against the reference's own committed vector: whisk.rs:416-456 comes out of the number 0 alone.  The cases
are those of tests/rng_cases.py, whose coverage the CPU test states.  Proof bytes are compared with the explicit-draw calls fed the model's
draws — those calls are pinned to the oracle and the reference vector by tests/test_gpu_whisk.py and tests/test_gpu_whisk_shuffle_batch.py."""
import ctypes
import os

import pytest

from tests import rng_cases as rc
from tests import stdrng_ref as sr
from tests.stdrng_ref import StdRng

pytestmark = pytest.mark.gpu

ELL = 28
BAD_POINT = bytes([0x80]) + bytes(46) + b"\x05"     # compressed, x = 5: not the x of a curve point


def _buf(b):
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


@pytest.fixture(scope="module")
def cpx():
    import curdleproofs_amd
    return curdleproofs_amd


@pytest.fixture(scope="module")
def plain(cpx):
    c = cpx.Context(0)          # no CRS: cpx_rng_fr needs none
    yield c
    c.close()


@pytest.fixture(scope="module")
def crs28(orc):
    return orc.generate_crs_points(ELL)


@pytest.fixture(scope="module", params=[{}, {"device_min_batch": 1}], ids=["default", "device_min_batch=1"])
def ctx28(request, cpx, crs28):
    """default options: 1 and 3 proofs are driven from the host, 57 run device-resident; device_min_batch = 1: all of them do"""
    c = cpx.Context(0, options=request.param)
    c.set_crs(ELL, crs28)
    yield c
    c.close()


def test_device_build_of_rng_check(tmp_path):
    """every function of rng.hpp on the device, bit for bit against the host twin and the model"""
    from curdleproofs_amd import build
    assert os.path.exists(build.check_path("rng_check")), "curdleproofs_amd/_lib/rng_check is missing: build() makes it"
    assert rc.list_operations(build.check_path("rng_check")) == rc.TABLE
    records = rc.check_records()
    dev = rc.run_check(build.check_path("rng_check"), records, tmp_path, "dev")
    twin = rc.run_check(rc.build_host_twin(tmp_path), records, tmp_path, "twin")
    total = sum(len(r) for _, r in records)
    assert rc.assert_rows(records, dev, twin, ("device", "host twin")) == total
    assert rc.assert_rows(records, dev, rc.check_expected(), ("device", "model")) == total


@pytest.mark.parametrize("case", range(len(rc.fr_cases())), ids=["n_each=%d%s" % (n, "" if i < len(rc.N_EACH) else "/searched") for i, (n, _) in enumerate(rc.fr_cases())])
def test_rng_fr(plain, cpx, case):
    n_each, states = rc.fr_cases()[case]
    for count in rc.COUNTS:
        want_out, want_states = rc.fr_expected(n_each, states[:count])
        st, out = _buf(b"".join(states[:count])), (ctypes.c_uint8 * (32 * n_each * count))()
        assert plain._L.cpx_rng_fr(plain._h, count, st, n_each, out) == cpx.CPX_OK
        assert bytes(out) == want_out, "count %d" % count
        assert bytes(st) == want_states, "count %d" % count
    assert plain.batch == 0


@pytest.mark.parametrize("ell", rc.SHUFFLE_ELLS)
def test_rng_shuffle_draws(cpx, orc, ell, crs28):
    c = cpx.Context(0)
    try:
        c.set_crs(ell, crs28 if ell == ELL else orc.generate_crs_points(ell))
        states = rc.shuffle_states(ell)
        want = rc.shuffle_expected(ell, states)
        count, nr = len(states), 3 * (ell + 4) + 9
        st = _buf(b"".join(states))
        perm, k, mb, rand = (ctypes.c_uint32 * (count * ell))(), (ctypes.c_uint8 * (32 * count))(), (ctypes.c_uint8 * (128 * count))(), (ctypes.c_uint8 * (32 * nr * count))()
        assert c._L.cpx_rng_shuffle_draws(c._h, count, st, perm, k, mb, rand) == cpx.CPX_OK
        assert list(perm) == [x for w in want for x in w[0]]
        assert bytes(k) == b"".join(w[1] for w in want) and bytes(mb) == b"".join(w[2] for w in want) and bytes(rand) == b"".join(w[3] for w in want)
        assert bytes(st) == b"".join(w[5] for w in want)
        # every output may be NULL: the states advance all the same
        st2 = _buf(b"".join(states))
        assert c._L.cpx_rng_shuffle_draws(c._h, count, st2, None, None, None, None) == cpx.CPX_OK and bytes(st2) == bytes(st)
        assert c.batch == 0
    finally:
        c.close()


@pytest.mark.parametrize("options", [{}, {"device_min_batch": 1}], ids=["host-driven", "device-resident"])
def test_reference_kat_from_the_number_zero(cpx, orc, whisk_kat, options):
    """whisk.rs:416-456: StdRng::seed_from_u64(0), 124 trackers from (k, r) draws, one shuffle proof, verified with eight more draws"""
    from curdleproofs_amd import whisk
    from curdleproofs_amd.rng import StdRng as Rng
    ell = 124
    kat = bytes.fromhex(whisk_kat["whisk_shuffle_proof_ell124"])
    c = cpx.Context(0, options=options)
    try:
        c.set_crs(ell, orc.generate_crs_points(ell))
        rng = Rng.seed_from_u64(0)
        kr = rng.fr(c, 2 * ell)                                   # generate_shuffle_trackers: per tracker k = Fr::rand, r = Fr::rand
        pre, _ = whisk.trackers_from_k_r(c, [kr[64 * i:64 * i + 32] for i in range(ell)], [kr[64 * i + 32:64 * i + 64] for i in range(ell)])
        model = StdRng.from_state(rng.state)
        perm, k, mb, rand, _ = model.shuffle_draws(ell)
        post, proof = whisk.generate_whisk_shuffle_proof(c, pre, rng=rng)
        assert proof == kat                                       # whisk.rs:455
        assert rng.state == model.state()
        post_explicit, proof_explicit = whisk.generate_whisk_shuffle_proof(c, pre, permutation=perm, k=k, vec_m_blinders=mb, rand=rand)
        assert post == post_explicit and proof_explicit == kat
        vrand = rng.fr(c, 8)
        assert vrand == model.fr(8) and whisk.is_valid_whisk_shuffle_proof(c, pre, post, proof, rand=vrand)
    finally:
        c.close()


class Shuffles:
    """57 lists of 28 trackers and a stream each, with the model's draws"""

    def __init__(self):
        parent = StdRng.seed_from_u64(77)
        self.count = 57
        kr = StdRng.seed_from_u64(78)
        self.ks = [kr.fr(1) for _ in range(self.count * ELL)]
        self.rs = [kr.fr(1) for _ in range(self.count * ELL)]
        self.states = []
        for i in range(self.count):
            ch = parent.split()
            ch.word_pos = i % 16                                   # (the shuffle starts at every offset)
            self.states.append(ch.state())
        self.draws = rc.shuffle_expected(ELL, tuple(self.states))

    def explicit(self, count):
        d = self.draws[:count]
        return dict(permutations=[x[0] for x in d], ks=[x[1] for x in d], vec_m_blinders=[x[2] for x in d], rands=[x[3] for x in d])


@pytest.fixture(scope="module")
def shuffles():
    return Shuffles()


def _pre_lists(ctx, sh, count):
    from curdleproofs_amd import whisk
    trk, _ = whisk.trackers_from_k_r(ctx, sh.ks[:count * ELL], sh.rs[:count * ELL])
    return [trk[ELL * i:ELL * (i + 1)] for i in range(count)]


@pytest.mark.parametrize("count", [1, 3, 57])
def test_rng_proofs_equal_the_explicit_draw_call(ctx28, shuffles, count):
    from curdleproofs_amd import whisk
    from curdleproofs_amd.rng import StdRng as Rng
    pre = _pre_lists(ctx28, shuffles, count)
    rngs = [Rng(s) for s in shuffles.states[:count]]
    got = whisk.generate_whisk_shuffle_proofs(ctx28, pre, rngs=rngs)
    assert ctx28.batch == count
    assert [r.state for r in rngs] == [d[5] for d in shuffles.draws[:count]]
    want = whisk.generate_whisk_shuffle_proofs(ctx28, pre, **shuffles.explicit(count))
    assert all(w is not None for w in want) and got == want
    post, proof = got[count - 1]
    assert whisk.is_valid_whisk_shuffle_proof(ctx28, pre[count - 1], post, proof)


def test_batch_prove_rng(ctx28, cpx, shuffles):
    """on the instances a shuffle call left loaded: cpx_batch_prove with the model's 3n + 9 draws against cpx_batch_prove_rng from the
    states as they stand behind the blinders"""
    from curdleproofs_amd import whisk
    count, nr = 3, 3 * (ELL + 4) + 9
    pre = _pre_lists(ctx28, shuffles, count)
    ex = shuffles.explicit(count)
    dense = [p[48:] for _, p in whisk.generate_whisk_shuffle_proofs(ctx28, pre, **ex)]
    assert ctx28.batch == count
    before = []
    for s in shuffles.states[:count]:
        m = StdRng.from_state(s)
        m.shuffle(ELL), m.fr(5)
        before.append(m.state())
    perm = (ctypes.c_uint32 * (count * ELL))(*[x for p in ex["permutations"] for x in p])
    k, mb = _buf(b"".join(ex["ks"])), _buf(b"".join(ex["vec_m_blinders"]))
    assert ctx28.prove_batch(perm, k, mb, _buf(b"".join(ex["rands"]))) == dense
    st, out = _buf(b"".join(before)), (ctypes.c_uint8 * (count * ctx28.proof_size))()
    assert ctx28._L.cpx_batch_prove_rng(ctx28._h, perm, k, mb, st, out) == cpx.CPX_OK
    psz = ctx28.proof_size
    assert [bytes(out)[psz * i:psz * (i + 1)] for i in range(count)] == dense
    assert bytes(st) == b"".join(d[5] for d in shuffles.draws[:count])


def test_undecodable_pre_tracker_advances_its_stream_by_the_shuffle_and_k_only(ctx28, shuffles):
    """whisk.rs:150-157: unzip_trackers fails after the permutation and k were drawn, before the blinders; the items beside it are untouched"""
    from curdleproofs_amd import whisk
    from curdleproofs_amd.rng import StdRng as Rng
    count = 3
    pre = _pre_lists(ctx28, shuffles, count)
    good = whisk.generate_whisk_shuffle_proofs(ctx28, pre, **shuffles.explicit(count))
    pre[1] = pre[1][:5] + [whisk.WhiskTracker(BAD_POINT, pre[1][5].k_r_G)] + pre[1][6:]
    rngs = [Rng(s) for s in shuffles.states[:count]]
    got = whisk.generate_whisk_shuffle_proofs(ctx28, pre, rngs=rngs)
    assert got[1] is None and got[0] == good[0] and got[2] == good[2]
    d = shuffles.draws
    assert [r.state for r in rngs] == [d[0][5], d[1][4], d[2][5]] and d[1][4] != d[1][5]
    with pytest.raises(whisk.SerializationError):
        whisk.generate_whisk_shuffle_proof(ctx28, pre[1], rng=Rng(shuffles.states[1]))


def test_argument_errors_write_nothing(ctx28, plain, cpx, shuffles):
    L = plain._L
    good = StdRng.seed_from_u64(4)
    late = StdRng(good.key, sr.POS_LIMIT).state()
    fill = bytes([0x5a])
    # cpx_rng_fr: a late state anywhere in the call, NULL with work to do, sizes beyond the limits; count = 0 and n_each = 0 are no-ops
    for states in (late, good.state() + late):
        st, out = _buf(states), _buf(fill * (64 * 2))
        assert L.cpx_rng_fr(plain._h, len(states) // 40, st, 2, out) == cpx.CPX_ERR_ARG
        assert bytes(st) == states and bytes(out) == fill * 128
    st, out = _buf(good.state()), _buf(fill * 64)
    assert L.cpx_rng_fr(plain._h, 1, None, 2, out) == cpx.CPX_ERR_ARG and L.cpx_rng_fr(plain._h, 1, st, 2, None) == cpx.CPX_ERR_ARG
    assert L.cpx_rng_fr(plain._h, 1, st, (1 << 20) + 1, out) == cpx.CPX_ERR_ARG and L.cpx_rng_fr(plain._h, (1 << 23) + 1, st, 1, out) == cpx.CPX_ERR_ARG
    assert L.cpx_rng_fr(plain._h, 0, None, 2, None) == cpx.CPX_OK and L.cpx_rng_fr(plain._h, 1, st, 0, out) == cpx.CPX_OK
    assert bytes(st) == good.state() and bytes(out) == fill * 64
    # the last valid position works
    st = _buf(StdRng(good.key, sr.POS_LIMIT - 1).state())
    assert L.cpx_rng_fr(plain._h, 1, st, 1, out) == cpx.CPX_OK and bytes(out)[:32] == StdRng(good.key, sr.POS_LIMIT - 1).fr(1)
    # cpx_rng_shuffle_draws: no CRS is a state error; a late state is an argument error
    st = _buf(good.state())
    assert L.cpx_rng_shuffle_draws(plain._h, 1, st, None, None, None, None) == cpx.CPX_ERR_STATE and bytes(st) == good.state()
    st, k = _buf(late), _buf(fill * 32)
    assert L.cpx_rng_shuffle_draws(ctx28._h, 1, st, None, k, None, None) == cpx.CPX_ERR_ARG and bytes(st) == late and bytes(k) == fill * 32
    assert L.cpx_rng_shuffle_draws(ctx28._h, 1, None, None, k, None, None) == cpx.CPX_ERR_ARG
    assert L.cpx_rng_shuffle_draws(ctx28._h, 0, None, None, None, None, None) == cpx.CPX_OK
    # cpx_whisk_generate_shuffle_proofs_rng and cpx_batch_prove_rng
    count = 2
    pre = b"".join(t.to_bytes() for lst in _pre_lists(ctx28, shuffles, count) for t in lst)
    rec = 48 + ctx28.proof_size
    states = shuffles.states[0] + late
    st, post, proofs = _buf(states), _buf(fill * (count * ELL * 96)), _buf(fill * (count * rec))
    status = (ctypes.c_int * count)(*([12345] * count))
    loaded = ctx28.batch
    assert L.cpx_whisk_generate_shuffle_proofs_rng(ctx28._h, count, _buf(pre), st, post, proofs, status) == cpx.CPX_ERR_ARG
    assert L.cpx_whisk_generate_shuffle_proofs_rng(ctx28._h, count, _buf(pre), None, post, proofs, status) == cpx.CPX_ERR_ARG
    assert L.cpx_whisk_generate_shuffle_proofs_rng(ctx28._h, 0, None, None, None, None, None) == cpx.CPX_OK
    assert bytes(st) == states and bytes(post) == fill * len(post) and bytes(proofs) == fill * len(proofs) and list(status) == [12345] * count
    assert ctx28.batch == loaded
    if loaded:
        perm = (ctypes.c_uint32 * (loaded * ELL))(*(list(range(ELL)) * loaded))
        k, mb = _buf(good.fr(loaded)), _buf(good.fr(4 * loaded))
        states = b"".join(StdRng(good.key, 100 * i).state() for i in range(loaded - 1)) + late
        st, out = _buf(states), _buf(fill * (loaded * ctx28.proof_size))
        assert L.cpx_batch_prove_rng(ctx28._h, perm, k, mb, st, out) == cpx.CPX_ERR_ARG
        assert L.cpx_batch_prove_rng(ctx28._h, perm, k, mb, None, out) == cpx.CPX_ERR_ARG
        assert bytes(st) == states and bytes(out) == fill * len(out)
