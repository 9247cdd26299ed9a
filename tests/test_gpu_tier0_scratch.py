"""The scratch contract of the tier-0 and batched Whisk calls (engine.hpp, Tier0 / ShuffleBufs / CallScope): a buffer that one large call grew
beyond 64 MiB is given back when that call ends, whichever buffer and whichever call.  Free-HBM figures of a shared GPU cannot be asserted on,
so the contract is read through the read-only key "tier0_scratch_bytes".  The sizes are the smallest that push a buffer over 64 MiB =
67 108 864 bytes (bytes per element: encoding 48, affine 96, Jacobian 144, status 1):

    decompress   1 400 000 points   bytes 67.2 MB and a0 134.4 MB cross it, status 1.4 MB stays
    normalize      700 000 points   jin 100.8 MB and a0 67.2 MB cross it, bytes 33.6 MB stays
    sum_jac        470 000 points   jin 67.7 MB crosses it

Inputs are one oracle point repeated, so the host builds them in milliseconds; expected values are the oracle's.  Every case runs on a
context of its own.  The single calls run the bodies of the many-calls with one task (Engine::msm_lists, Engine::fold_lanes): their launch
statistics are pinned at the end."""
import pytest

pytestmark = pytest.mark.gpu

FR, AFF, JAC = 32, 96, 144
R_ = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
KEEP = 64 << 20
LARGE = {"decompress": 1400000, "normalize": 700000, "sum_jac": 470000}


def _wire(orc, ints):
    return orc.fr_from_canonical_bytes(b"".join((v % R_).to_bytes(32, "little") for v in ints))


class Point:
    """one seeded oracle point in every form the cases need, and small operands for the calls that follow a large one"""

    def __init__(self, orc):
        rng = orc.rng(20261020)
        self.aff = rng.g1_affine(1)
        k = rng.fr(1)
        self.jac = orc.g1_msm(orc.g1_scale(self.aff, orc.fr_inv(k)), k)                    # P again, with a Z of the oracle's making
        self.neg_jac = orc.g1_msm(orc.g1_scale(self.aff, _wire(orc, [R_ - 1])), _wire(orc, [1]))
        self.comp = orc.g1_compress(self.aff)
        self.identity = orc.g1_msm(self.aff, _wire(orc, [0]))
        assert orc.g1_to_affine(self.jac) == self.aff and orc.g1_compress_jac(self.jac) == self.comp
        assert orc.g1_eq_jac(orc.g1_add_jac(self.jac, self.neg_jac), self.identity)
        self.bases, self.scalars = rng.g1_affine(33), rng.fr(33)
        self.msm = orc.g1_msm(self.bases, self.scalars)
        self.pl, self.pr, self.gamma = rng.g1_affine(16), rng.g1_affine(16), rng.fr(1)
        self.fold = orc.g1_fold(self.pl, self.pr, self.gamma)


@pytest.fixture(scope="module")
def point(orc):
    return Point(orc)


def _large_call(c, orc, point, call):
    n = LARGE[call]
    if call == "decompress":
        assert 48 * n > KEEP and AFF * n > KEEP and n < KEEP
        got = c.decompress(point.comp * n, check_subgroup=False)
        assert len(got) == AFF * n and got[:AFF] == point.aff and got[-AFF:] == point.aff
    elif call == "normalize":
        assert JAC * n > KEEP and AFF * n > KEEP and 48 * n < KEEP
        aff, comp = c.normalize(point.jac * n, compressed=True)
        assert len(aff) == AFF * n and aff[:AFF] == point.aff and aff[-AFF:] == point.aff
        assert len(comp) == 48 * n and comp[:48] == point.comp and comp[-48:] == point.comp
    else:
        assert JAC * n > KEEP and n % 2 == 0
        total, is_identity = c.sum_jac((point.jac + point.neg_jac) * (n // 2))          # P and -P in equal numbers
        assert is_identity and orc.g1_eq_jac(total, point.identity)


@pytest.mark.parametrize("call", list(LARGE))
def test_a_large_call_gives_its_buffers_back(orc, point, call):
    """at the parent commit the decompress case left bytes, status and a0 (more than 200 MB) resident for the life of the context"""
    import curdleproofs_amd as cpx
    c = cpx.Context(0)
    try:
        _large_call(c, orc, point, call)
        left = c.get_option("tier0_scratch_bytes")
        print("%s of %d points: tier0_scratch_bytes = %d" % (call, LARGE[call], left))
        assert left < KEEP
    finally:
        c.close()


def test_a_small_call_after_a_large_one_is_served_from_regrown_scratch(orc, point):
    import curdleproofs_amd as cpx
    c = cpx.Context(0)
    try:
        _large_call(c, orc, point, "decompress")
        assert orc.g1_eq_jac(c.msm(point.bases, point.scalars), point.msm)
        assert c.fold(point.pl, point.pr, point.gamma) == point.fold
        assert 0 < c.get_option("tier0_scratch_bytes") < KEEP
    finally:
        c.close()


def test_the_key_is_read_only_and_bounded(orc, point):
    import curdleproofs_amd as cpx
    c = cpx.Context(0)
    try:
        assert c.get_option("tier0_scratch_bytes") == 0
        assert orc.g1_eq_jac(c.msm(point.bases, point.scalars), point.msm)
        assert 0 < c.get_option("tier0_scratch_bytes") < KEEP
        with pytest.raises(cpx.CpxError) as refused:
            c.set_option("tier0_scratch_bytes", 1)
        assert refused.value.code == cpx.CPX_ERR_ARG
    finally:
        c.close()


def test_statistics_of_the_single_calls(orc, point):
    import curdleproofs_amd as cpx
    names = ("k_msm_tblw<2, true>", "k_reduce_sets", "k_msm_tail", "k_finalize", "k_smul")
    c = cpx.Context(0)
    try:
        c.set_profiling(True)
        assert orc.g1_eq_jac(c.msm(point.bases, point.scalars), point.msm)
        assert {k: c.stat(k)["launches"] for k in names} == {"k_msm_tblw<2, true>": 1, "k_reduce_sets": 1, "k_msm_tail": 1, "k_finalize": 0, "k_smul": 0}
        assert c.stat("k_msm_tblw<2, true>")["units"] == 33 and c.stat("k_msm_tail")["units"] == 1
        c.reset_stats()
        assert c.fold(point.pl, point.pr, point.gamma) == point.fold
        assert c.stat("k_smul")["launches"] == 1 and c.stat("k_smul")["units"] == 16
        assert c.stat("k_smul_quad")["launches"] == 0                       # cpx_g1_fold keeps the one-lane kernel (option fold_quad_max)
        c.reset_stats()
        c.set_option("msm_endo_min", 64)                                    # 33 points are below it: the windowed accumulation
        assert orc.g1_eq_jac(c.msm(point.bases, point.scalars), point.msm)
        assert c.stat("k_msm_accw")["launches"] == 1 and c.stat("k_msm_tblw<2, true>")["launches"] == 0
    finally:
        c.close()
