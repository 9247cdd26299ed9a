"""GPU tests of the grouped verifier (cpx_batch_verify_grouped, cpx_whisk_verify_shuffle_proofs_grouped; include/cpx.h,
curdleproofs_amd/csrc/locate_plan.hpp): one verdict per proof from the fused check stopped at its groups, and a check of their own only for
the proofs of a failing group.  Every verdict list is compared with cpx_batch_verify on the same proofs (8 factors), every mutated proof with
the oracle; `n_rechecked`, which is deterministic, shows that only the failing groups are rechecked.  Each case runs on both verifier paths:
default options (the host drives batches below 56 proofs) and a context with device_min_batch = 1.  ell = 28 unless stated; option
locate_groups_max = 4 cuts ten proofs into groups of 3, 3, 3 and 1."""
import pytest

from tests.test_gpu_parity import THROUGHPUT, _proof_offsets

pytestmark = pytest.mark.gpu

ELL = 28
B10 = 10
GROUPS10 = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9]]
POSITIONS = (0, 5, 9)                        # first proof of a full group, last proof of a full group, the lone proof of the short group
MUTATIONS = ("neighbour", "z_k", "L_C1")
BAD_FACTOR = b"\xff" * 32                    # limbs >= r


class Base:
    """three oracle instances at ell = 28, repeated over a batch (proof p belongs to instance p % 3), and every mutated proof with the
    oracle's verdict"""

    def __init__(self, orc, ell=ELL, seeds=(31, 32, 33)):
        self.ell = ell
        self.crs = orc.generate_crs_points(ell)
        self.insts = [orc.make_instance(ell, s, self.crs) for s in seeds]
        off = _proof_offsets(ell)
        rng = orc.rng(20262)
        scalar = orc.fr_to_canonical_bytes(rng.fr(1))
        point = orc.g1_compress(rng.g1_affine(1))
        self.mutated = {}
        for i, x in enumerate(self.insts):
            good = x["proof"]
            o_z, o_l = off["z_k"], off["L_C"] + 48
            forms = {"neighbour": self.insts[(i + 1) % len(self.insts)]["proof"], "z_k": good[:o_z] + scalar + good[o_z + 32:],
                     "L_C1": good[:o_l] + point + good[o_l + 48:]}
            for name, bad in forms.items():
                assert bad != good
                assert orc.verify(ell, self.crs, x["vec_R"], x["vec_S"], x["vec_T"], x["vec_U"], x["M"], bad, x["verifier_rand"]) == 0, (i, name)
                self.mutated[(i, name)] = bad
        # an instance whose vec_T[0] is the identity (curdleproofs.rs:218): rejected whatever the proof says
        x = dict(self.insts[1])
        x["vec_T"] = bytes(96) + x["vec_T"][96:]
        assert orc.verify(ell, self.crs, x["vec_R"], x["vec_S"], x["vec_T"], x["vec_U"], x["M"], x["proof"], x["verifier_rand"]) == 0
        self.t0_identity = x

    def inst(self, p):
        return self.insts[p % len(self.insts)]

    def load(self, c, B, replace=None):
        replace = replace or {}
        rows = [replace.get(p, self.inst(p)) for p in range(B)]
        c.set_crs(self.ell, self.crs)
        c.load_batch(*(b"".join(r[k] for r in rows) for k in ("vec_R", "vec_S", "vec_T", "vec_U", "M")))

    def proofs(self, B, wrong=None):
        """wrong: {position: mutation name}"""
        out = [self.inst(p)["proof"] for p in range(B)]
        for p, name in (wrong or {}).items():
            out[p] = self.mutated[(p % len(self.insts), name)]
        return out

    def vrand(self, B):
        return b"".join(self.inst(p)["verifier_rand"] for p in range(B))


@pytest.fixture(scope="module")
def base(orc):
    return Base(orc)


@pytest.fixture(scope="module")
def contexts():
    import curdleproofs_amd as cpx
    made = {}

    def get(name):
        if name not in made:
            opts = {"host_driven": {}, "device_resident": {"device_min_batch": 1}, "throughput_host": dict(THROUGHPUT),
                    "throughput_device": dict(THROUGHPUT, device_min_batch=1)}[name]
            made[name] = cpx.Context(0, options=opts)
        return made[name]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(params=["host_driven", "device_resident"])
def c(request, contexts):
    c = contexts(request.param)
    if request.param == "host_driven":
        assert c.get_option("device_min_batch") > 18
    return c


def _check(c, orc, proofs, vrand, seed, want_rechecked, groups_max=4, fused=True):
    """grouped verdicts == cpx_batch_verify's, n_rechecked as expected, and the fused call accepts exactly when every verdict is CPX_OK"""
    import curdleproofs_amd as cpx
    c.set_option("locate_groups_max", groups_max)
    frand = orc.rng(seed).fr(12 * len(proofs))
    got, rechecked = c.verify_batch_grouped(proofs, frand)
    print("grouped: %d proofs, not CPX_OK %s, n_rechecked %d (want %d)" % (len(got), {p: v for p, v in enumerate(got) if v}, rechecked, want_rechecked))
    assert got == c.verify_batch(proofs, vrand)
    assert rechecked == want_rechecked
    if fused:
        assert c.verify_batch_fused(proofs, frand) == all(v == cpx.CPX_OK for v in got)
    assert c.batch == len(proofs)
    return got


# ---- 1. all valid ----
def test_all_valid_rechecks_nothing(c, orc, base):
    import curdleproofs_amd as cpx
    base.load(c, B10)
    for seed in (1, 2):                                  # fresh factors give the same verdicts
        assert _check(c, orc, base.proofs(B10), base.vrand(B10), seed, 0) == [cpx.CPX_OK] * B10


# ---- 2. a wrong proof by position and by mutation ----
def _wrong_by_position(c, orc, base):
    import curdleproofs_amd as cpx
    base.load(c, B10)
    for pos in POSITIONS:
        size = len(next(g for g in GROUPS10 if pos in g))
        for name in MUTATIONS:
            got = _check(c, orc, base.proofs(B10, {pos: name}), base.vrand(B10), 10 + pos, size)
            assert got == [cpx.CPX_ERR_VERIFY if p == pos else cpx.CPX_OK for p in range(B10)], (pos, name)
    # two victims in two groups: both groups; two victims in one group: that group once
    for victims, want in (((0, 5), 6), ((3, 5), 3), ((5, 9), 4)):
        got = _check(c, orc, base.proofs(B10, {p: "z_k" for p in victims}), base.vrand(B10), 77, want)
        assert got == [cpx.CPX_ERR_VERIFY if p in victims else cpx.CPX_OK for p in range(B10)], victims


def test_wrong_proof_by_position(c, orc, base):
    _wrong_by_position(c, orc, base)


# ---- 3. flags ----
def test_flagged_proofs(c, orc, base):
    import curdleproofs_amd as cpx
    OK, VER, DES = cpx.CPX_OK, cpx.CPX_ERR_VERIFY, cpx.CPX_ERR_DESERIALIZE
    broken = lambda proof: bytes([proof[0] ^ 0x80]) + proof[1:]
    base.load(c, B10)
    # an undecodable proof contributes nothing: its neighbours are not rechecked
    proofs = base.proofs(B10)
    proofs[4] = broken(proofs[4])
    assert _check(c, orc, proofs, base.vrand(B10), 3, 0, fused=False) == [DES if p == 4 else OK for p in range(B10)]
    # ... beside a wrong proof in its group: only the flag-free proofs of the group are rechecked
    proofs = base.proofs(B10, {3: "z_k"})
    proofs[4] = broken(proofs[4])
    assert _check(c, orc, proofs, base.vrand(B10), 4, 2, fused=False) == [VER if p == 3 else DES if p == 4 else OK for p in range(B10)]
    # groups made only of undecodable proofs: a full one and the short one
    proofs = base.proofs(B10)
    for p in (3, 4, 5, 9):
        proofs[p] = broken(proofs[p])
    assert _check(c, orc, proofs, base.vrand(B10), 5, 0, fused=False) == [DES if p in (3, 4, 5, 9) else OK for p in range(B10)]
    # vec_T[0] is the identity: rejected as by cpx_batch_verify; the proof keeps its scalars, so the rest of its group is rechecked
    base.load(c, B10, {4: base.t0_identity})
    assert _check(c, orc, base.proofs(B10), base.vrand(B10), 6, 2) == [VER if p == 4 else OK for p in range(B10)]


# ---- 4. one group of 18 x 631 points ----
@pytest.fixture(scope="module")
def base124(orc):
    return Base(orc, 124, (0, 1, 2))


def test_one_group_of_many_points(c, orc, base124):
    import curdleproofs_amd as cpx
    B = 18
    base124.load(c, B)
    assert _check(c, orc, base124.proofs(B), base124.vrand(B), 7, 0, groups_max=1) == [cpx.CPX_OK] * B
    got = _check(c, orc, base124.proofs(B, {B - 1: "neighbour"}), base124.vrand(B), 8, B, groups_max=1)
    assert got == [cpx.CPX_OK] * (B - 1) + [cpx.CPX_ERR_VERIFY]


# ---- 5. default grouping on the device path, and the plan cache ----
def test_default_grouping_on_the_device_path(contexts, orc, base):
    import curdleproofs_amd as cpx
    c = contexts("host_driven")                          # default options: 600 proofs run device-resident
    one = Base.__new__(Base)
    one.__dict__.update(base.__dict__)
    one.insts = base.insts[:1]                           # copies of one instance
    one.mutated = {(0, "z_k"): base.mutated[(0, "z_k")]}
    assert c.get_option("device_min_batch") <= 598
    B = 600
    one.load(c, B)
    victims = (0, 299, 599)
    proofs = one.proofs(B, {p: "z_k" for p in victims})
    want = [cpx.CPX_ERR_VERIFY if p in victims else cpx.CPX_OK for p in range(B)]
    assert _check(c, orc, proofs, one.vrand(B), 9, 9, groups_max=256, fused=False) == want      # G = 3, NT = 200
    frand = orc.rng(91).fr(12 * B)
    seen = []
    for groups_max in (256, 1, 256):                     # the cached plan follows the option on the loaded batch
        c.set_option("locate_groups_max", groups_max)
        seen.append(c.verify_batch_grouped(proofs, frand))
    assert [v for v, _ in seen] == [want] * 3 and [n for _, n in seen] == [9, B, 9]
    B = 598                                              # the last group holds one proof
    one.load(c, B)
    got = _check(c, orc, one.proofs(B, {597: "z_k"}), one.vrand(B), 10, 1, groups_max=256, fused=False)
    assert got == [cpx.CPX_OK] * 597 + [cpx.CPX_ERR_VERIFY]


# ---- 6. the throughput forms of the kernels ----
@pytest.mark.parametrize("name", ["throughput_host", "throughput_device"])
def test_wrong_proof_by_position_on_the_throughput_kernels(contexts, orc, base, name):
    _wrong_by_position(contexts(name), orc, base)


# ---- 7. the fused call is untouched by a grouped call in between ----
def test_fused_partial_sum_is_unchanged_by_a_grouped_call(c, orc, base):
    base.load(c, B10)
    c.set_option("locate_groups_max", 4)
    proofs = base.proofs(B10, {5: "L_C1"})
    frand = orc.rng(12).fr(12 * B10)
    before = c.verify_batch_fused_partial(proofs, frand)
    c.verify_batch_grouped(proofs, orc.rng(13).fr(12 * B10))
    after = c.verify_batch_fused_partial(proofs, frand)
    assert before == after and before[1] == 0 and orc.g1_compress_jac(before[0])[0] != 0xc0


# ---- 7b. what the shared staging of the accumulated check (check_plan.hpp) decides for every mode ----
def test_an_undecodable_proof_contributes_nothing_in_any_mode_on_either_path(contexts, orc, base):
    import curdleproofs_amd as cpx
    OK, VER, DES = cpx.CPX_OK, cpx.CPX_ERR_VERIFY, cpx.CPX_ERR_DESERIALIZE
    identity = bytes([0xc0]) + bytes(47)
    broken = lambda proof: bytes([proof[0] ^ 0x80]) + proof[1:]
    frand = orc.rng(18).fr(12 * B10)
    sums = {}
    for name in ("host_driven", "device_resident"):
        c = contexts(name)
        base.load(c, B10)
        c.set_option("locate_groups_max", 4)
        # proof 4 undecodable, the rest valid: the fused sum is the identity and the proof is counted; the per-proof call names it
        proofs = base.proofs(B10)
        proofs[4] = broken(proofs[4])
        jac, invalid = c.verify_batch_fused_partial(proofs, frand)
        assert invalid == 1 and bytes(orc.g1_compress_jac(jac)) == identity, name
        assert c.verify_batch(proofs, base.vrand(B10)) == [DES if p == 4 else OK for p in range(B10)], name
        # ... beside a wrong proof: only the undecodable one is counted, and the wrong one's sum is the same on both paths
        proofs = base.proofs(B10, {3: "z_k"})
        proofs[4] = broken(proofs[4])
        jac, invalid = c.verify_batch_fused_partial(proofs, frand)
        sums[name] = bytes(orc.g1_compress_jac(jac))
        print("%s: n_invalid %d, partial sum %s" % (name, invalid, sums[name].hex()))
        assert invalid == 1 and sums[name] != identity, name
        assert c.verify_batch(proofs, base.vrand(B10)) == [VER if p == 3 else DES if p == 4 else OK for p in range(B10)], name
    assert sums["host_driven"] == sums["device_resident"]


# ---- 8. arguments ----
def test_arguments(c, orc, base):
    import curdleproofs_amd as cpx
    base.load(c, B10)
    proofs = base.proofs(B10)
    frand = orc.rng(14).fr(12 * B10)
    for bad in (bytes(32), BAD_FACTOR):
        for at in (0, 12 * B10 - 1):
            with pytest.raises(cpx.CpxError) as e:
                c.verify_batch_grouped(proofs, frand[:32 * at] + bad + frand[32 * (at + 1):])
            assert e.value.code == cpx.CPX_ERR_ARG
            assert c.batch == B10
    fresh = cpx.Context(0)
    try:
        fresh.set_crs(base.ell, base.crs)
        with pytest.raises(cpx.CpxError) as e:
            fresh.verify_batch_grouped([], b"")
        assert e.value.code == cpx.CPX_ERR_STATE and fresh.batch == 0
    finally:
        fresh.close()


# ---- 9. Whisk ----
@pytest.fixture(scope="module")
def whisk_data(orc):
    from tests.test_gpu_whisk_shuffle_batch import Data
    return Data(orc)


def test_whisk_grouped_equals_the_per_proof_call(c, orc, whisk_data):
    from curdleproofs_amd import whisk
    from tests.test_gpu_whisk_shuffle_batch import NI, _answers, _trackers
    d = whisk_data
    c.set_crs(28, d.crs)
    c.set_option("locate_groups_max", 4)                 # 12 items: four groups of three
    pre, post = [_trackers(x) for x in d.vpre], [_trackers(x) for x in d.vpost]
    rng = orc.rng(15)
    got, rechecked = whisk.are_valid_whisk_shuffle_proofs_grouped(c, pre, post, d.vproofs, [rng.fr(12) for _ in range(NI)])
    assert c.batch == NI
    ref = whisk.are_valid_whisk_shuffle_proofs(c, pre, post, d.vproofs, d.vrand)
    print("whisk grouped: %s n_rechecked %d" % (_answers(got), rechecked))
    assert _answers(got) == _answers(ref) == d.want[False]
    assert set(_answers(got)) == {1, 0, -1}
    assert 0 < rechecked <= NI


def test_whisk_grouped_accepts_the_reference_vector(c, orc, whisk_kat):
    from curdleproofs_amd import whisk
    from tests.test_gpu_whisk_shuffle_batch import _trackers, _zip_compress
    ell = 124
    crs = orc.generate_crs_points(ell)
    rng = orc.rng(0)                                     # whisk.rs:416-424, as tests/test_gpu_whisk_shuffle_batch.py builds the vector's shuffle
    gen = orc.g1_generator()
    kr = [(rng.fr(1), rng.fr(1)) for _ in range(ell)]
    vec_R = orc.g1_scale(gen * ell, b"".join(r for _, r in kr))
    vec_S = orc.g1_scale(vec_R, b"".join(k for k, _ in kr))
    perm, k, mb = rng.shuffle(ell), rng.fr(1), rng.fr(4)
    vec_T, vec_U, _ = orc.shuffle_permute_and_commit_input(ell, crs, vec_R, vec_S, perm, k, mb)
    proof = bytes.fromhex(whisk_kat["whisk_shuffle_proof_ell124"])
    assert len(proof) == 4496
    c.set_crs(ell, crs)
    got, rechecked = whisk.are_valid_whisk_shuffle_proofs_grouped(c, [_trackers(_zip_compress(orc, vec_R, vec_S))], [_trackers(_zip_compress(orc, vec_T, vec_U))],
                                                                 [proof], [orc.rng(16).fr(12)])
    assert got == [True] and rechecked == 0


# ---- 10. the profile ----
def test_profile_shows_one_group_sum_and_a_second_stage_only_when_needed(contexts, orc, base):
    endo = "k_msm_tblw<2, true>"
    for name, sums in (("device_resident", 1), ("host_driven", 0)):      # the host-driven path sums the CRS scalars on the host
        c = contexts(name)
        base.load(c, B10)
        c.set_option("locate_groups_max", 4)
        c.set_profiling(True)
        try:
            for wrong, want_rechecked, stages in ((None, 0, 1), ({5: "z_k"}, 3, 2)):
                c.reset_stats()
                _, rechecked = c.verify_batch_grouped(base.proofs(B10, wrong), orc.rng(17).fr(12 * B10))
                assert rechecked == want_rechecked
                assert c.stat("k_vs_crs_sum_groups")["launches"] == sums, name
                assert c.stat(endo)["launches"] == stages and c.stat("k_msm_tail")["launches"] == stages, name
                assert c.stat(endo)["units"] > 0
        finally:
            c.set_profiling(False)
