"""GPU parity tests: the HIP path behind the C-ABI (include/cpx.h) against the CPU oracle on the same
seeded inputs — bit-exact (integer work).  Run on the MI355X box with `pytest -m gpu`."""
import hashlib
import os

import pytest

pytestmark = pytest.mark.gpu

FR, AFF, JAC = 32, 96, 144


@pytest.fixture(scope="module")
def ctx():
    import curdleproofs_amd as cpx
    return cpx.Context(0)


def _same_point(orc, jac_a, jac_b):
    return orc.g1_compress_jac(jac_a) == orc.g1_compress_jac(jac_b)


def test_native_library_loaded():
    import curdleproofs_amd as cpx
    L = cpx.load_library()
    assert L.cpx_device_count() >= 1, "no HIP device visible: the product path has no CPU fallback"


def test_quad_cooperative_formulas_match_one_lane_formulas():
    """g1_28_quad.hpp (point additions / doublings spread over the four lanes of a quad: the latency kernels) against the
    one-lane formulas of g1_28.hpp on the device: generic sums, P + P, P - P, identity operands, doublings.  The check is
    scripts/micro/quad_micro.hip, built with the library (curdleproofs_amd/build.py)."""
    import subprocess
    from curdleproofs_amd.build import SELFCHECK
    assert os.path.exists(SELFCHECK), "run python -m curdleproofs_amd.build"
    r = subprocess.run([SELFCHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout + r.stderr


# (1112: the verifier's points per proof, one round of the bucket-list wave since round 5; 4096 / 4097 / 9000: the 14-bit point index of a
# one-window-per-half round at its limit, one point beyond it, and a task of three rounds)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 31, 32, 33, 64, 128, 252, 256, 257, 300, 600, 1112, 4096, 4097, 9000])
def test_msm_matches_oracle(ctx, orc, n):
    rng = orc.rng(1000 + n)
    bases = rng.g1_affine(n)
    scalars = rng.fr(n)
    got = ctx.msm(bases, scalars)
    want = orc.g1_msm(bases, scalars)
    assert _same_point(orc, got, want)


@pytest.mark.parametrize("endo_min", [1, 64], ids=["bucket_list_path", "windowed_accumulation_k_msm_accw"])
def test_msm_below_64_points_on_both_paths(orc, endo_min):
    """util::msm with fewer than 64 points: since round 6 the endomorphism bucket-list path by default (option msm_endo_min = 1: 0.72 ms per call against
    1.4 ms), before that the plain windowed accumulation k_msm_accw, which stays reachable through the option.  Both against the oracle, n = 0 and the
    edge scalars included."""
    import curdleproofs_amd as cpx
    c = cpx.Context(0, options={"msm_endo_min": endo_min})
    try:
        assert cpx.Context(0).get_option("msm_endo_min") == 1
        for n in (0, 1, 2, 3, 5, 17, 40, 63):
            rng = orc.rng(7100 + n)
            bases, scalars = rng.g1_affine(n), rng.fr(n)
            assert _same_point(orc, c.msm(bases, scalars), orc.g1_msm(bases, scalars)), n
        rng = orc.rng(7200)
        bases = rng.g1_affine(6)
        r_minus_1 = (0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001 - 1).to_bytes(32, "little")
        scalars = b"".join(orc.fr_from_canonical_bytes(x) for x in ((0).to_bytes(32, "little"), (1).to_bytes(32, "little"), r_minus_1,
                                                                   (1 << 128).to_bytes(32, "little"), ((1 << 128) - 1).to_bytes(32, "little"), (255).to_bytes(32, "little")))
        bases = bases[:96] + bytes(96) + bases[192:]   # an identity base among them
        assert _same_point(orc, c.msm(bases, scalars), orc.g1_msm(bases, scalars))
    finally:
        c.close()


def test_msm_edge_cases(ctx, orc):
    rng = orc.rng(7)
    n = 40
    bases = bytearray(rng.g1_affine(n))
    scalars = bytearray(rng.fr(n))
    ident = bytes(AFF)
    # identity bases (the G1Affine::zero() padding of curdleproofs.rs:141-155), zero and unit scalars,
    # repeated bases, a base and its scalar twice (forces P + P inside a bucket), r - 1
    bases[0:AFF] = ident
    bases[5 * AFF:6 * AFF] = ident
    scalars[2 * FR:3 * FR] = bytes(FR)
    scalars[3 * FR:4 * FR] = orc.fr_from_u64(1)
    bases[7 * AFF:8 * AFF] = bases[6 * AFF:7 * AFF]
    scalars[7 * FR:8 * FR] = scalars[6 * FR:7 * FR]
    rm1 = (0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001 - 1).to_bytes(32, "little")
    scalars[9 * FR:10 * FR] = orc.fr_from_canonical_bytes(rm1)
    bases[11 * AFF:12 * AFF] = bases[10 * AFF:11 * AFF]
    scalars[11 * FR:12 * FR] = orc.fr_from_canonical_bytes(rm1)   # -P beside ...
    scalars[10 * FR:11 * FR] = orc.fr_from_u64(1)                 # ... +P : cancels
    got = ctx.msm(bytes(bases), bytes(scalars))
    want = orc.g1_msm(bytes(bases), bytes(scalars), naive=True)
    assert _same_point(orc, got, want)
    # all-identity / all-zero MSM is the identity
    z = ctx.msm(ident * 5, rng.fr(5))
    assert orc.g1_compress_jac(z)[0] == 0xC0
    z = ctx.msm(rng.g1_affine(5), bytes(FR * 5))
    assert orc.g1_compress_jac(z)[0] == 0xC0


def test_msm_endomorphism_path_edge_cases(ctx, orc):
    """n >= 64 goes through the endomorphism split + radix-256 bucket lists (k_msm_tblw<2, true>, the verifier's kernel):
    scalars at the edges of the split (0, 1, r - 1, z^2, z^2 / 2, (r +- 1) / 2, 2^128 - 1, all-0x80 digit bytes), identity
    bases, a repeated (base, scalar) pair, a cancelling pair, and more points than one list round holds."""
    R_ = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    z2 = 0xd201000000010000 ** 2
    rng = orc.rng(77)
    n = 200
    bases = bytearray(rng.g1_affine(n))
    scalars = bytearray(rng.fr(n))
    special = [0, 1, 2, R_ - 1, R_ - 2, z2, z2 - 1, z2 + 1, z2 // 2, z2 // 2 + 1, (R_ - 1) // 2, (R_ + 1) // 2, (1 << 128) - 1, 1 << 127,
               int.from_bytes(b"\x80" * 31 + b"\x00", "little") % R_, int.from_bytes(b"\x7f" * 31 + b"\x00", "little") % R_, 255, 256, 128, 127,
               (z2 * (z2 // 2)) % R_, (z2 * 128 + 128) % R_]
    for i, v in enumerate(special):
        scalars[(20 + i) * FR:(21 + i) * FR] = orc.fr_from_canonical_bytes(v.to_bytes(32, "little"))
    ident = bytes(AFF)
    bases[0:AFF] = ident
    bases[25 * AFF:26 * AFF] = ident
    bases[7 * AFF:8 * AFF] = bases[6 * AFF:7 * AFF]           # P, s twice: P + P inside a bucket
    scalars[7 * FR:8 * FR] = scalars[6 * FR:7 * FR]
    bases[11 * AFF:12 * AFF] = bases[10 * AFF:11 * AFF]       # +P and -P: cancels
    scalars[10 * FR:11 * FR] = orc.fr_from_u64(1)
    scalars[11 * FR:12 * FR] = orc.fr_from_canonical_bytes((R_ - 1).to_bytes(32, "little"))
    got = ctx.msm(bytes(bases), bytes(scalars))
    want = orc.g1_msm(bytes(bases), bytes(scalars), naive=True)
    assert _same_point(orc, got, want)
    # all-zero scalars / all-identity bases
    assert orc.g1_compress_jac(ctx.msm(rng.g1_affine(100), bytes(FR * 100)))[0] == 0xC0
    assert orc.g1_compress_jac(ctx.msm(ident * 100, rng.fr(100)))[0] == 0xC0
    # several list rounds per wave (272 points fit one round), one scalar repeated (a single bucket takes everything)
    n = 1500
    bases = rng.g1_affine(n)
    scalars = rng.fr(n)
    assert _same_point(orc, ctx.msm(bases, scalars), orc.g1_msm(bases, scalars))
    same = scalars[:FR] * n
    assert _same_point(orc, ctx.msm(bases, same), orc.g1_msm(bases, same))


def test_msm_length_mismatch_is_an_error(ctx, orc):
    rng = orc.rng(3)
    with pytest.raises(ValueError):   # util.rs:20 assert_eq!(points.len(), scalars.len())
        ctx.msm(rng.g1_affine(3), rng.fr(2))


def test_msm_from_projective(ctx, orc):
    rng = orc.rng(11)
    n = 8
    aff = rng.g1_affine(n)
    # make non-trivial Jacobian representatives: P_i = msm([P_i, P_i'], [s, 0])
    jac = b"".join(orc.g1_msm(aff[i * AFF:(i + 1) * AFF], orc.fr_from_u64(3 + i)) for i in range(n))
    scalars = rng.fr(n)
    assert _same_point(orc, ctx.msm_from_projective(jac, scalars), orc.g1_msm_jac(jac, scalars))


@pytest.mark.parametrize("half", [1, 2, 3, 64, 128, 300])
def test_fold_matches_oracle(ctx, orc, half):
    rng = orc.rng(2000 + half)
    PL, PR, gamma = bytearray(rng.g1_affine(half)), bytearray(rng.g1_affine(half)), rng.fr(1)
    if half >= 3:   # identity operands on either side (blinder slots of vec_T / vec_U)
        PL[0:AFF] = bytes(AFF)
        PR[AFF:2 * AFF] = bytes(AFF)
    assert ctx.fold(bytes(PL), bytes(PR), gamma) == orc.g1_fold(bytes(PL), bytes(PR), gamma)


def test_fold_cancellation(ctx, orc):
    # PL = -gamma*PR  ->  identity out
    rng = orc.rng(5)
    PR, gamma = rng.g1_affine(4), rng.fr(1)
    r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    g = int.from_bytes(orc.fr_to_canonical_bytes(gamma), "little")
    ng = orc.fr_from_canonical_bytes(((r - g) % r).to_bytes(32, "little"))
    PL = orc.g1_scale(PR, ng)
    assert ctx.fold(PL, PR, gamma) == bytes(AFF * 4) == orc.g1_fold(PL, PR, gamma)


@pytest.mark.parametrize("n", [1, 5, 256, 260])
def test_scale_matches_oracle(ctx, orc, n):
    rng = orc.rng(3000 + n)
    P = rng.g1_affine(n)
    per_elem = rng.fr(n)
    assert ctx.scale(P, per_elem) == orc.g1_scale(P, per_elem)
    if n > 1:
        shared = rng.fr(1)
        assert ctx.scale(P, shared) == orc.g1_scale(P, shared)


def test_scale_and_fold_on_curve_points_outside_the_subgroup(orc):
    """cpx_g1_scale / cpx_g1_fold on points of E(Fp) that are NOT in the order-r subgroup (what the hash-to-curve CRS ceremony multiplies by
    the cofactor, tests/crs.rs:32-38): with option scale_any_point = 1 (plain double-and-add) the results equal the oracle's double-and-add
    for full-width scalars; the default form (endomorphism split, include/cpx.h states the subgroup precondition) still agrees for the
    cofactor itself, whose split has no upper half, and for points inside the subgroup either setting gives the same bytes."""
    import hashlib
    import curdleproofs_amd as cpx
    from curdleproofs_amd import params as pr
    from curdleproofs_amd.crs import COFACTOR
    c = cpx.Context(0)
    cands = []
    for inc in range(64):
        hsh = hashlib.sha256(b"outside the subgroup" + inc.to_bytes(8, "big")).digest()
        x = sum(int.from_bytes(hsh[8 * i:8 * i + 8], "big") << (64 * i) for i in range(4))
        cands.append(bytes([0x80 | (x >> 376)]) + (x & ((1 << 376) - 1)).to_bytes(47, "big"))
    aff, status = c.decompress_status(b"".join(cands), check_subgroup=False)
    pts = b"".join(aff[AFF * j:AFF * (j + 1)] for j in range(64) if status[j] == 0)
    n = len(pts) // AFF
    assert n >= 16
    comp = c.normalize(b"".join(pts[AFF * t:AFF * (t + 1)] + pr.fp_to_wire(1) for t in range(n)), compressed=True)[1]
    assert all(s == 2 for s in c.decompress_status(comp, check_subgroup=True)[1])          # on the curve, outside the subgroup
    rng = orc.rng(4242)
    big = rng.fr(n)                                                                         # full-width scalars: the split would use phi
    c.set_option("scale_any_point", 1)
    assert c.scale(pts, big) == orc.g1_scale(pts, big)
    shared = rng.fr(1)
    assert c.scale(pts, shared) == orc.g1_scale(pts, shared)
    h = pr.fr_to_wire(COFACTOR)
    cleared = c.scale(pts, h)
    assert cleared == orc.g1_scale(pts, h)
    half = n // 2
    assert c.fold(pts[:half * AFF], pts[half * AFF:2 * half * AFF], shared) == orc.g1_fold(pts[:half * AFF], pts[half * AFF:2 * half * AFF], shared)
    inside = rng.g1_affine(8)
    k8 = rng.fr(8)
    plain = c.scale(inside, k8)
    c.set_option("scale_any_point", 0)
    assert c.scale(pts, h) == cleared                                                       # q = 0: nothing of phi is used
    assert c.scale(inside, k8) == plain == orc.g1_scale(inside, k8)
    assert c.scale(pts, big) != orc.g1_scale(pts, big)                                      # the documented precondition is a real one


def test_normalize_compress_decompress(ctx, orc):
    rng = orc.rng(17)
    n = 70
    aff = rng.g1_affine(n)
    jac = b"".join(orc.g1_msm(aff[i * AFF:(i + 1) * AFF], orc.fr_from_u64(2 + i)) for i in range(n))
    jac = jac[:JAC * 3] + bytes(JAC) + jac[JAC * 4:]   # a Z = 0 identity in the middle
    a, c = ctx.normalize(jac, compressed=True)
    assert a == orc.g1_to_affine(jac)
    assert c == orc.g1_compress_jac(jac)
    assert ctx.decompress(c) == a
    assert ctx.decompress(c) == orc.g1_decompress(c)


def test_decompress_rejects_bad_encodings(ctx, orc):
    import curdleproofs_amd as cpx
    good = orc.g1_compress(orc.g1_generator())
    for bad in (bytes(48),                                  # compression flag missing
                bytes([0x40]) + bytes(47),                  # infinity flag without the compression flag
                bytes([0x9F]) + b"\xff" * 47):              # x >= p
        with pytest.raises(cpx.CpxError):
            ctx.decompress(bad)
    # (encodings with the infinity flag set and other bits beside it: test_noncanonical_infinity_encodings_follow_the_option)
    # a point on the curve but outside the r-torsion subgroup must fail the subgroup check only
    x = 0
    for cand in range(1, 200):
        enc = bytes([0x80]) + cand.to_bytes(47, "big")
        try:
            orc.g1_decompress(enc)
        except ValueError:
            try:
                ctx.decompress(enc, check_subgroup=False)
            except cpx.CpxError:
                continue   # not on the curve at all
            with pytest.raises(cpx.CpxError):
                ctx.decompress(enc, check_subgroup=True)
            x = cand
            break
    assert x, "no on-curve/out-of-subgroup sample found"
    assert ctx.decompress(good) == orc.g1_generator()


def test_crs_sums(ctx, orc):
    ell = 28
    crs = orc.generate_crs_points(ell)
    ctx.set_crs(ell, crs)
    assert ctx.crs_sums() == orc.crs_sums(ell, crs)


def test_accumulator_matches_reference_semantics(ctx, orc):
    # msm_accumulator.rs:82-106 test_accumulator, n = 4, plus a failing variant
    import curdleproofs_amd as cpx
    rng = orc.rng(0)
    n = 4
    V, x = rng.g1_affine(n), rng.fr(n)
    C = orc.g1_msm(V, x)
    acc = cpx.MsmAccumulator(ctx)
    acc.accumulate_check(C, x, V, rng.fr(1))
    acc.accumulate_check(C, x, V, rng.fr(1))
    acc.verify()
    acc = cpx.MsmAccumulator(ctx)
    acc.accumulate_check(C, x, V, rng.fr(1))
    acc.accumulate_check(orc.g1_msm(V, rng.fr(n)), x, V, rng.fr(1))
    with pytest.raises(cpx.ProofError):
        acc.verify()


def test_accumulator_shared_bases_identity_and_projective_lhs(ctx, orc):
    """msm_accumulator.rs:38-68 beyond the reference's own n = 4 test: checks of different lengths over the SAME bases (their
    scalars merge under one key, :47-51), the identity as a base (the G1Affine::zero() padding of curdleproofs.rs:141-155),
    n = ell + 4 = 32, left-hand sides handed over as non-normalised Jacobian points (Z != 1) and as the point at infinity.
    Expected verdict = every individual relation C_i == msm(V_i, x_i) holds (checked with the oracle's MSM)."""
    import curdleproofs_amd as cpx
    rng = orc.rng(4711)
    n = 32
    V = bytearray(rng.g1_affine(n))
    V[3 * AFF:4 * AFF] = bytes(AFF)                        # identity base (also a map key)
    V[9 * AFF:10 * AFF] = V[8 * AFF:9 * AFF]               # the same base twice inside one check
    V = bytes(V)
    checks = []
    for m in (n, 10, 1, n):                                # different lengths over prefixes of the same base vector
        x = rng.fr(m)
        C = orc.g1_msm(V[:m * AFF], x)                     # Jacobian, Z != 1
        checks.append((C, x, V[:m * AFF]))
    zero_x = bytes(FR * 5)
    checks.append((bytes(JAC), zero_x, V[:5 * AFF]))       # O == msm(V, 0): Z = 0 left-hand side
    for C, x, Vs in checks:
        assert _same_point(orc, C, orc.g1_msm(Vs, x))

    def run(cs):
        acc = cpx.MsmAccumulator(ctx)
        for C, x, Vs in cs:
            acc.accumulate_check(C, x, Vs, rng.fr(1))
        acc.verify()

    run(checks)
    # one wrong left-hand side (C_1 + C_2 instead of C_1) anywhere rejects
    bad = list(checks)
    bad[1] = (orc.g1_add_jac(checks[1][0], checks[2][0]), checks[1][1], checks[1][2])
    with pytest.raises(cpx.ProofError):
        run(bad)
    # a wrong scalar on the identity base is invisible (x * O = O): still accepted, as in the reference
    x0 = bytearray(checks[0][1])
    x0[3 * FR:4 * FR] = rng.fr(1)
    run([(checks[0][0], bytes(x0), checks[0][2])] + checks[1:])
    # a zero random factor is refused (it would drop the check)
    acc = cpx.MsmAccumulator(ctx)
    with pytest.raises(cpx.CpxError) as e:
        acc.accumulate_check(checks[0][0], checks[0][1], checks[0][2], bytes(FR))
    assert e.value.code == cpx.CPX_ERR_ARG


def test_crs_not_enough_points(ctx, orc):
    import curdleproofs_amd as cpx
    crs = orc.generate_crs_points(28)
    with pytest.raises(cpx.CpxError) as e:                 # crs.rs:40-42 "not enough points"
        ctx.set_crs(28, crs[:-AFF])
    assert e.value.code == cpx.CPX_ERR_ARG
    ctx.set_crs(28, crs + crs[:AFF])                       # surplus points are ignored (the reference slices)
    assert ctx.crs_sums() == orc.crs_sums(28, crs)


def _prove_and_check(ctx, orc, ell, seeds):
    import curdleproofs_amd as cpx
    crs = orc.generate_crs_points(ell)
    ctx.set_crs(ell, crs)
    insts = [orc.make_instance(ell, s, crs) for s in seeds]
    cat = lambda key: b"".join(i[key] for i in insts)
    ctx.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
    perms = [x for i in insts for x in i["permutation"]]
    proofs = ctx.prove_batch(perms, cat("k"), cat("vec_m_blinders"), cat("prover_rand"))
    for inst, proof in zip(insts, proofs):
        assert len(proof) == len(inst["proof"])
        assert proof == inst["proof"], "proof bytes differ from the oracle's at byte %d" % next(
            i for i in range(len(proof)) if proof[i] != inst["proof"][i])
    verdicts = ctx.verify_batch(proofs, cat("verifier_rand"))
    assert verdicts == [cpx.CPX_OK] * len(insts)
    return crs, insts, proofs


def test_prove_verify_ell28_readme_example(ctx, orc, oracle_vectors):
    # BASELINE config 1 (README.md:76-118): ell = 28, StdRng seed 0
    crs, insts, proofs = _prove_and_check(ctx, orc, 28, [0])
    assert hashlib.sha256(proofs[0]).hexdigest() == oracle_vectors["28"]["proof_sha256"]


def test_prove_matches_reference_kat_ell124(ctx, orc, whisk_kat):
    # whisk.rs:416-456: the GPU prover must reproduce the reference's own 4496-byte vector.
    # Inputs are regenerated by the oracle's StdRng model exactly as the reference test draws them.
    import curdleproofs_amd as cpx
    ell = 124
    kat = bytes.fromhex(whisk_kat["whisk_shuffle_proof_ell124"])
    crs = orc.generate_crs_points(ell)
    rng = orc.rng(0)
    # generate_shuffle_trackers: (k, r) pairs -> r_G = r*G, k_r_G = k*r_G
    gen = orc.g1_generator()
    vec_R, vec_S = b"", b""
    for _ in range(ell):
        k, r = rng.fr(1), rng.fr(1)
        rG = orc.g1_scale(gen, r)
        vec_R += rG
        vec_S += orc.g1_scale(rG, k)
    perm = rng.shuffle(ell)
    k = rng.fr(1)
    mb = rng.fr(4)
    vec_T, vec_U, M = orc.shuffle_permute_and_commit_input(ell, crs, vec_R, vec_S, perm, k, mb)
    assert orc.g1_compress_jac(M) == kat[:48]
    rand = rng.fr(3 * (ell + 4) + 9)
    ctx.set_crs(ell, crs)
    ctx.load_batch(vec_R, vec_S, vec_T, vec_U, M)
    proof = ctx.prove_batch(perm, k, mb, rand)[0]
    assert proof == kat[48:]
    assert ctx.verify_batch([proof], rng.fr(8)) == [cpx.CPX_OK]


def test_shuffle_permute_and_commit_input_matches_oracle_and_kat(ctx, orc, whisk_kat):
    # util.rs:83-106 on the product API (curdleproofs_amd.util): k*R, k*S, permutation, M = msm(G, sigma) + msm(H, blinders).
    # Inputs as in whisk.rs:416-456, so M must compress to the first 48 bytes of the reference's shuffle-proof vector.
    from curdleproofs_amd import util
    ell = 124
    kat = bytes.fromhex(whisk_kat["whisk_shuffle_proof_ell124"])
    crs = orc.generate_crs_points(ell)
    rng = orc.rng(0)
    gen = orc.g1_generator()
    vec_R, vec_S = b"", b""
    for _ in range(ell):
        k, r = rng.fr(1), rng.fr(1)
        rG = orc.g1_scale(gen, r)
        vec_R += rG
        vec_S += orc.g1_scale(rG, k)
    perm = rng.shuffle(ell)
    k = rng.fr(1)
    mb = rng.fr(4)
    want_T, want_U, want_M = orc.shuffle_permute_and_commit_input(ell, crs, vec_R, vec_S, perm, k, mb)
    got_T, got_U, got_M = util.shuffle_permute_and_commit_input(ctx, crs, ell, vec_R, vec_S, perm, k, mb)
    assert got_T == want_T and got_U == want_U
    assert util.serialize_g1projective_vec(ctx, got_M) == kat[:48] == orc.g1_compress_jac(want_M)
    # (de)serialisation helpers round-trip (util.rs:116-133)
    comp = util.serialize_g1projective_vec(ctx, got_M + want_M)
    assert util.deserialize_g1projective_vec(ctx, comp, 2) == orc.g1_to_affine(got_M) * 2
    with pytest.raises(ValueError):
        util.msm(ctx, crs[:96 * 3], mb)   # util.rs:20 assert_eq!(points.len(), scalars.len())
    assert util.get_verification_scalars_bitstring(4, 2) == [[], [1], [0], [0, 1]]


def test_prove_verify_ell252_batch(ctx, orc, oracle_vectors):
    # BASELINE config 2 (single ell = 252 instance, seed 0) inside a small batch (config 4 recipe: seed = index)
    crs, insts, proofs = _prove_and_check(ctx, orc, 252, [0, 1, 2])
    assert hashlib.sha256(proofs[0]).hexdigest() == oracle_vectors["252"]["proof_sha256"]


def test_prove_verify_ell60(ctx, orc):
    # curdleproofs.rs:336-378 (N = 64, ell = 60): whole-shuffle round trip, here bit-exact against the oracle
    _prove_and_check(ctx, orc, 60, [0, 7])


def test_prove_verify_batch40_ell28(ctx, orc):
    # 40 independent instances (BASELINE config 4 recipe: instance i from StdRng(i)): large enough for the engine's
    # batch paths (host-driven protocol on the spin team below 56 proofs, multi-chunk host loops; the device-resident form of this
    # test runs in test_engine_variants_stay_bit_exact); every proof must equal
    # the oracle's bytes and verify
    _prove_and_check(ctx, orc, 28, list(range(100, 140)))


def test_prove_verify_ell1020_single(ctx, orc, oracle_vectors):
    # BASELINE config 3 (ell = 1020, n = 1024, 10 rounds, seed 0): proof bytes equal the oracle's, 5888 B
    crs, insts, proofs = _prove_and_check(ctx, orc, 1020, [0])
    assert len(proofs[0]) == 5888
    assert hashlib.sha256(proofs[0]).hexdigest() == oracle_vectors["1020"]["proof_sha256"]


def test_verify_rejects_mutated_instances(ctx, orc):
    # curdleproofs.rs:427-470 test_bad_shuffle_arguments, N = 128: the four negative mutations
    import curdleproofs_amd as cpx
    ell = 124
    crs = orc.generate_crs_points(ell)
    ctx.set_crs(ell, crs)
    inst = orc.make_instance(ell, 0, crs)
    R, S, T, U, M, proof, vr = (inst[k] for k in ("vec_R", "vec_S", "vec_T", "vec_U", "M", "proof", "verifier_rand"))
    rng = orc.rng(99)

    def verdict(R_, S_, T_, U_, M_):
        ctx.load_batch(R_, S_, T_, U_, M_)
        v = ctx.verify_batch([proof], vr)[0]
        assert v == {1: cpx.CPX_OK, 0: cpx.CPX_ERR_VERIFY}[orc.verify(ell, crs, R_, S_, T_, U_, M_, proof, vr)]
        return v

    assert verdict(R, S, T, U, M) == cpx.CPX_OK
    assert verdict(S, R, T, U, M) == cpx.CPX_ERR_VERIFY                       # swapped inputs
    p2 = rng.shuffle(ell)
    perm_pts = lambda v: b"".join(v[i * AFF:(i + 1) * AFF] for i in p2)
    assert verdict(R, S, perm_pts(T), perm_pts(U), M) == cpx.CPX_ERR_VERIFY   # another permutation
    Mk = orc.g1_msm(orc.g1_to_affine(M), inst["k"])
    assert verdict(R, S, T, U, Mk) == cpx.CPX_ERR_VERIFY                      # wrong permutation commitment
    k2 = rng.fr(1)
    assert verdict(R, S, orc.g1_scale(T, k2), orc.g1_scale(U, k2), M) == cpx.CPX_ERR_VERIFY   # another randomiser
    assert verdict(R, S, bytes(AFF) + T[AFF:], U, M) == cpx.CPX_ERR_VERIFY    # vec_T[0] is the identity (:218)


def test_verify_rejects_corrupted_proof_bytes(ctx, orc):
    import curdleproofs_amd as cpx
    ell = 28
    crs = orc.generate_crs_points(ell)
    ctx.set_crs(ell, crs)
    inst = orc.make_instance(ell, 3, crs)
    ctx.load_batch(inst["vec_R"], inst["vec_S"], inst["vec_T"], inst["vec_U"], inst["M"])
    proof = bytearray(inst["proof"])
    assert ctx.verify_batch([bytes(proof)], inst["verifier_rand"]) == [cpx.CPX_OK]
    # swap two proof points (still valid encodings): verification error
    a, b = bytes(proof[0:48]), bytes(proof[48:96])
    bad = bytes(b + a + proof[96:])
    assert ctx.verify_batch([bad], inst["verifier_rand"]) == [cpx.CPX_ERR_VERIFY]
    assert orc.verify(ell, crs, inst["vec_R"], inst["vec_S"], inst["vec_T"], inst["vec_U"], inst["M"], bad, inst["verifier_rand"]) == 0
    # a scalar >= r : deserialisation error
    psz = len(proof)
    bad = bytes(proof[:psz - 32]) + b"\xff" * 32
    assert ctx.verify_batch([bad], inst["verifier_rand"]) == [cpx.CPX_ERR_DESERIALIZE]
    assert orc.verify(ell, crs, inst["vec_R"], inst["vec_S"], inst["vec_T"], inst["vec_U"], inst["M"], bad, inst["verifier_rand"]) == -1
    # a point that is not on the curve
    bad = bytes([0x80]) + bytes(46) + b"\x05" + bytes(proof[48:])
    v = ctx.verify_batch([bad], inst["verifier_rand"])[0]
    o = orc.verify(ell, crs, inst["vec_R"], inst["vec_S"], inst["vec_T"], inst["vec_U"], inst["M"], bad, inst["verifier_rand"])
    assert (v == cpx.CPX_ERR_DESERIALIZE and o == -1) or (v == cpx.CPX_ERR_VERIFY and o == 0)


@pytest.mark.parametrize("copies", [1, 60], ids=["host_driven", "device_resident"])
def test_noncanonical_infinity_encodings_follow_the_option(orc, copies):
    """Point encodings whose infinity flag is set but which are not 0xc0 || 0^47 (sort flag set, x bits set).  ark-bls12-381 ^0.4's
    `read_g1_compressed` — behind curdleproofs.rs:312-323 / whisk.rs:313-320 — takes the infinity flag at its word (include/cpx.h states
    the source of that knowledge and its limits): the point IS the identity, and what the verifier hashes is the identity's canonical
    serialisation.  Option strict_infinity = 0 (default) must therefore give such a proof exactly the verdict the oracle gives it in its
    ^0.4 mode — the verdict of the same proof with the canonical 0xc0 encoding in that place, i.e. VerificationError —, and
    strict_infinity = 1 the oracle's strict verdict, SerializationError.  Tier 0 (cpx_g1_decompress) follows the same option.
    Per-proof verdicts and the fused verifier, host-driven and device-resident path."""
    import curdleproofs_amd as cpx
    ell = 28
    crs = orc.generate_crs_points(ell)
    inst = orc.make_instance(ell, 5, crs)
    proof = inst["proof"]
    L = 5
    canon = bytes([0xc0]) + bytes(47)
    variants = [bytes([0xe0]) + bytes(47), bytes([0xc0]) + bytes(46) + b"\x01", bytes([0xff]) + b"\xff" * 47, bytes([0xc0, 0x01]) + bytes(46)]
    # places: A (the first point), L_C[1] (inside the IPA block, after the r_p scalar), R_U[last] (the last point)
    q_lc1 = 9 + 2 + 1
    places = [0, 48 * q_lc1 + 32, len(proof) - 32 - 48]
    cases = [(off, v) for off in places for v in variants]
    put = lambda off, enc: proof[:off] + enc + proof[off + 48:]
    c = cpx.Context(0)
    try:
        c.set_crs(ell, crs)
        B = copies * len(cases)
        rep = lambda key: inst[key] * B
        c.load_batch(rep("vec_R"), rep("vec_S"), rep("vec_T"), rep("vec_U"), rep("M"))
        vr = inst["verifier_rand"] * B
        V = lambda o: {1: cpx.CPX_OK, 0: cpx.CPX_ERR_VERIFY, -1: cpx.CPX_ERR_DESERIALIZE}[o]
        over = lambda pr: orc.verify(ell, crs, inst["vec_R"], inst["vec_S"], inst["vec_T"], inst["vec_U"], inst["M"], pr, inst["verifier_rand"])
        assert c.get_option("strict_infinity") == 0
        for strict in (0, 1, 0):
            c.set_option("strict_infinity", strict)
            orc.set_strict_infinity(bool(strict))
            try:
                bad = [put(off, v) for off, v in cases] * copies
                want = [V(over(b)) for b in bad[:len(cases)]] * copies
                if strict:
                    assert set(want) == {cpx.CPX_ERR_DESERIALIZE}
                else:   # the identity in that place: the verdict of the canonical encoding there
                    assert want[:len(cases)] == [V(over(put(off, canon))) for off, _ in cases] and set(want) == {cpx.CPX_ERR_VERIFY}
                assert c.verify_batch(bad, vr) == want
                good_but_one = [proof] * (B - 1) + [bad[0]]
                frand = orc.rng(77).fr(12 * B)
                assert c.verify_batch_fused([proof] * B, frand) and not c.verify_batch_fused(good_but_one, frand)
                for v in variants:
                    if strict:
                        with pytest.raises(cpx.CpxError):
                            c.decompress(v)
                        with pytest.raises(ValueError):
                            orc.g1_decompress(v)
                    else:
                        assert c.decompress(v) == bytes(AFF) == orc.g1_decompress(v)
                assert c.decompress(canon) == bytes(AFF)
            finally:
                orc.set_strict_infinity(False)
    finally:
        c.close()


def test_not_power_of_two_is_an_error(ctx, orc):
    import curdleproofs_amd as cpx
    with pytest.raises(cpx.CpxError) as e:   # inner_product_argument.rs:116 assert!(n.is_power_of_two())
        ctx.set_crs(27, orc.generate_crs_points(27))
    assert e.value.code == cpx.CPX_ERR_NOT_POW2


@pytest.mark.parametrize("wpw", [2, 4, 8, 16, 32])
def test_table_msm_window_groupings_reproduce_kat(wpw, orc, whisk_kat, oracle_vectors):
    # k_msm_tblw<WPW>: the launcher picks the windows-per-wave grouping from the grid size, so small batches only
    # reach WPW = 8.  Pin the other instantiations (a context of its own with the option set) on the reference KAT.
    import curdleproofs_amd as cpx
    c = cpx.Context(0, options={"tbw_wpw": wpw})
    try:
        assert c.get_option("tbw_wpw") == wpw
        test_prove_matches_reference_kat_ell124(c, orc, whisk_kat)
        test_prove_verify_ell252_batch(c, orc, oracle_vectors)
    finally:
        c.close()


def test_fused_batch_verifier_config5(ctx, orc):
    # BASELINE config 5: one accumulated MSM over all proofs of the batch (all-or-nothing).  The verdict must equal
    # the AND of the oracle's per-proof verdicts; the partial sum of a valid batch is the point at infinity.
    import curdleproofs_amd as cpx
    ell = 28
    seeds = [0, 1, 2, 3, 4]
    crs, insts, proofs = _prove_and_check(ctx, orc, ell, seeds)
    rand = orc.rng(4242).fr(12 * len(seeds))
    part, bad = ctx.verify_batch_fused_partial(proofs, rand)
    assert bad == 0
    assert orc.g1_compress_jac(part) == bytes([0xc0]) + bytes(47)          # identity
    assert ctx.verify_batch_fused(proofs, rand)
    # the same partial split over two "GPUs": halves of the batch, partials added like the all-gather step does
    cat = lambda key, sel: b"".join(insts[i][key] for i in sel)
    halves = []
    for sel in ([0, 1], [2, 3, 4]):
        ctx.load_batch(cat("vec_R", sel), cat("vec_S", sel), cat("vec_T", sel), cat("vec_U", sel), cat("M", sel))
        pj, b = ctx.verify_batch_fused_partial([proofs[i] for i in sel], rand[:12 * 32 * len(sel)])
        assert b == 0
        halves.append(pj)
    assert ctx.sum_jac(b"".join(halves))[1]
    # one wrong proof anywhere rejects the batch: proof 3 verified against instance 2's proof bytes
    ctx.load_batch(cat("vec_R", range(5)), cat("vec_S", range(5)), cat("vec_T", range(5)), cat("vec_U", range(5)), cat("M", range(5)))
    wrong = list(proofs)
    wrong[3] = proofs[2]
    want = all(orc.verify(ell, crs, insts[i]["vec_R"], insts[i]["vec_S"], insts[i]["vec_T"], insts[i]["vec_U"], insts[i]["M"], wrong[i],
                          insts[i]["verifier_rand"]) == 1 for i in range(5))
    assert want is False
    assert not ctx.verify_batch_fused(wrong, rand)
    part, bad = ctx.verify_batch_fused_partial(wrong, rand)
    assert orc.g1_compress_jac(part) != bytes([0xc0]) + bytes(47)
    # a corrupted point encoding is reported as structurally invalid
    broken = bytearray(proofs[1])
    broken[0] ^= 0x80
    wrong = list(proofs)
    wrong[1] = bytes(broken)
    part, bad = ctx.verify_batch_fused_partial(wrong, rand)
    assert bad == 1 and not ctx.verify_batch_fused(wrong, rand)


@pytest.mark.parametrize("ell,nproofs", [(124, 3)])
def test_fused_batch_verifier_many_points(ctx, orc, ell, nproofs):
    # 18 proofs x 631 points in one task of the endomorphism bucket-list kernel (several list rounds per wave)
    crs, insts, proofs = _prove_and_check(ctx, orc, ell, list(range(nproofs)) * 6)
    rand = orc.rng(7).fr(12 * len(proofs))
    assert ctx.verify_batch_fused(proofs, rand)
    wrong = list(proofs)
    wrong[-1] = proofs[0]
    assert not ctx.verify_batch_fused(wrong, rand)


# The bench runs 2048 proofs per engine context: its launchers then pick k_msm_fix<16, 16>, k_msm_tblw<32, false>, the
# thread-per-group reductions (k_reduce_sets / k_reduce_groups) and the thread-per-request k_finalize_ranges, none of which
# a batch of a few proofs reaches.  THROUGHPUT_ENV moves every switch-over so that small batches run exactly those
# instantiations (kernels.hip: msm_fix_windows_per_wave, msm_tblw_windows_per_wave, launch_reduce_sets,
# launch_finalize_ranges, launch_msm_tail).
THROUGHPUT = {"fix_min_waves": 1, "tbw_wpw": 32, "reduce_wave_max": 0, "finalize_wave_max": 0, "tail_wave_max": 0, "table_quad_max": 0, "decompress_quad_max": 0}
VARIANTS = {
    "fix8": {"fix_bits": 8},
    "fix19": {"fix_bits": 19},                                  # 14 windows of 19 bits, 122 GB table at ell = 252 (falls back to 16 when HBM is short)
    "fix19_late_rounds_throughput_kernels": {"fix_bits": 19, "late_min_batch": 1, "device_min_batch": 1, "fix_min_waves": 1, "reduce_wave_max": 0},
    "device_resident": {"device_min_batch": 1},                 # (log rounds fused, round.hip: the default up to 256 proofs: fused_rounds_max, fused_smsm_max)
    # the log rounds as ONE launch each (round.hip: MSM waves that reduce their own accumulators, the last arriver of a proof finalises, hashes,
    # draws the challenge and folds) in every wave shape the launcher offers, and switched off (the chain of separate kernels)
    "device_resident_unfused_rounds": {"device_min_batch": 1, "fused_rounds_max": 0, "smul_quad_max": 0},   # (and the one-lane k_smul for the T_2 commitments)
    "fused_rounds_combined_waves": {"device_min_batch": 1, "fused_combine": 1, "fused_fix_wpw": 8},
    "fused_rounds_four_windows_per_fixed_wave": {"device_min_batch": 1, "fused_fix_wpw": 4},
    "fused_rounds_whole_tasks_per_wave": {"device_min_batch": 1, "fused_fix_wpw": 16, "fused_tbl_wpw": 32, "fused_combine": 0},
    "fused_rounds_eight_windows_per_table_wave": {"device_min_batch": 1, "fused_tbl_wpw": 8, "fused_combine": 0},
    "fused_rounds_separate_fixed_and_table_waves": {"device_min_batch": 1, "fused_combine": 0},
    "host_driven": {"device_min_batch": 1000000},
    "throughput_kernels": THROUGHPUT,
    "throughput_kernels_device_resident": dict(THROUGHPUT, device_min_batch=1, fused_rounds_max=0),
    "four_point_slices_host_driven": {"tbw_slices": 4, "device_min_batch": 1000000},
    "two_point_slices_thread_tail": {"tbw_slices": 2, "tail_wave_max": 0},
    "plain_streams_wave_kernels_everywhere": {"cu_mask": 0, "reduce_wave_max": 1000000, "finalize_wave_max": 1000000},
    # the last four log rounds on materialised folded bases (late.hip: k_late_fix, k_late_uniform, k_late_tables, k_late_msm), which only
    # batches of >= late_min_batch proofs take by default, forced onto single proofs and small batches; and switched off
    "late_rounds_on_small_batches": {"late_min_batch": 1, "device_min_batch": 1},
    "late_rounds_on_small_batches_fix8": {"late_min_batch": 1, "device_min_batch": 1, "fix_bits": 8},
    "late_rounds_one_lane_per_output": {"late_min_batch": 1, "device_min_batch": 1, "late_slices": 1},
    "late_rounds_eight_lanes_per_output": {"late_min_batch": 1, "device_min_batch": 1, "late_slices": 8, "tail_wave_max": 0},
    "late_rounds_off": {"late_rounds": 0, "device_min_batch": 1},
    "lane_per_transcript_prefix": {"transcript_lane_min_batch": 1, "device_min_batch": 1},   # k_transcript_step1_lane: one lane per proof hashes the instance
    "phase1_in_one_piece": {"p1_split": 0, "device_min_batch": 1},   # A inside phase 1 (default: phase 1 without A before the transcript prefix is awaited, A behind it)
    "rs_as_two_tasks": {"rs_pairs": 0, "device_min_batch": 1},     # R = <a, vec_R>, S = <a, vec_S> as separate tasks (default: one wave serves both)
    # the wave-per-transcript prefix without SIMDs of its own (default up to 256 proofs: k_transcript_step1<true> on a high-priority stream)
    "prefix_shares_its_simds": {"transcript_excl_max": 0, "device_min_batch": 1},
    # every stream's work in line on the main stream (measurement aid of bench.py): table stream, side stream, prefix stream
    "serial_streams_device_resident": {"serial_streams": 1, "device_min_batch": 1},
}


def _variant_checks(c, orc, whisk_kat, oracle_vectors):
    test_prove_matches_reference_kat_ell124(c, orc, whisk_kat)
    test_verify_rejects_mutated_instances(c, orc)
    test_fused_batch_verifier_config5(c, orc)
    test_prove_verify_ell252_batch(c, orc, oracle_vectors)
    test_same_scalar_relations_are_checked(c, orc)
    test_prove_verify_batch40_ell28(c, orc)
    test_verify_rejects_corrupted_proof_bytes(c, orc)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_engine_variants_stay_bit_exact(name, orc, whisk_kat, oracle_vectors):
    # the 8-bit fixed-base table, the device-resident protocol (step kernels of protocol.hip; normally used from 56 proofs per
    # batch on) forced on single proofs, the host-driven protocol forced on a batch of 40, and the throughput instantiations
    # of the MSM / reduction / finalisation kernels, the point slices of the bucket-list MSM (msm_tblw_slices: by default only
    # tasks of >= 512 points of a lone proof are sliced) and the latency kernels forced onto every batch size
    # are alternative engine configurations, selected per context through cpx_ctx_set_option; all must reproduce the reference
    # KAT (whisk.rs:416-456), the oracle's bytes at ell = 28 / 252 and the oracle's verdicts
    import curdleproofs_amd as cpx
    c = cpx.Context(0, options=VARIANTS[name])
    try:
        for k, v in VARIANTS[name].items():
            assert c.get_option(k) == v
        seen = []   # the radix of the fixed-base table actually in use after every set_crs of the checks
        plain_set_crs = c.set_crs
        c.set_crs = lambda ell, pts: (plain_set_crs(ell, pts), seen.append((ell, c.get_option("fix_bits_effective"))))[0]
        _variant_checks(c, orc, whisk_kat, oracle_vectors)
        if "fix_bits" in VARIANTS[name]:
            # the CONFIGURED radix is not the one in use when set_crs fell back (19 -> 16 -> 8 when free HBM is short, e.g. beside other
            # contexts' tables in this process): a variant that silently ran another table pins nothing
            fell_back = sorted({(e, b) for e, b in seen if b != VARIANTS[name]["fix_bits"]})
            if fell_back:
                pytest.skip("fixed-base table fell back (free HBM) at (ell, bits) = %s: the %d-bit kernels did not run there" % (fell_back, VARIANTS[name]["fix_bits"]))
            if VARIANTS[name]["fix_bits"] == 19 and "late_min_batch" in VARIANTS[name]:
                c.set_profiling(True)
                c.reset_stats()
                test_prove_verify_batch40_ell28(c, orc)
                assert c.stat("k_msm_fix<19, 7>")["launches"] > 0 and c.stat("k_late_fix")["launches"] > 0
    finally:
        c.close()


@pytest.mark.parametrize("ell,seeds,late_m", [(28, [0, 1, 2], 0), (60, [0, 1], 0), (1020, [0], 0), (1020, [0], 16), (1020, [0], 64), (508, [0], 0), (508, [0], 64),
                                              (252, [0, 1], 32), (252, [0], 64), (124, [0], 64), (60, [0, 1], 32)])
def test_late_rounds_on_materialised_bases_other_sizes(orc, oracle_vectors, ell, seeds, late_m):
    """late.hip at the sizes the variant checks do not reach: ell = 28 (n = 32: two points per materialised base, first late round
    = round 1), ell = 60, ell = 1020 (default there: m = 32 materialised bases per family, five late rounds, one lane per output; m = 16: 64
    points per base, 2048-entry digit lists; m = 64: six late rounds, two k_late_uniform waves per proof), ell = 508 (default m = 32; m = 64), and the deeper shapes forced onto n = 256 / 128 / 64 (late_m; an m the proof is too short for falls back).  Bytes == oracle."""
    import curdleproofs_amd as cpx
    c = cpx.Context(0, options={"late_min_batch": 1, "device_min_batch": 1, "late_m": late_m})
    try:
        c.set_profiling(True)
        crs, insts, proofs = _prove_and_check(c, orc, ell, seeds)
        n, L = ell + 4, (ell + 4).bit_length() - 1
        m = late_m or (32 if n >= 512 else 16)
        while m > 16 and m >= n:
            m //= 2
        # the late rounds ran, as many as the shape says: log2(m) rounds x 2 arguments
        assert c.stat("k_late_uniform")["launches"] == 1 and c.stat("k_late_msm")["launches"] == 2 * min(m.bit_length() - 1, L - 1)
        if str(ell) in oracle_vectors:
            assert hashlib.sha256(proofs[0]).hexdigest() == oracle_vectors[str(ell)]["proof_sha256"]
    finally:
        c.close()


def test_late_rounds_at_default_options_every_proof_matches_oracle(orc):
    """The late rounds of late.hip as a large batch takes them by DEFAULT (>= 2048 proofs per context; the variant tests force them onto
    small batches): 2048 independent ell = 28 instances on one context with default options — k_late_* must have run (kernel
    statistics), every proof equals the oracle's bytes, every verdict the oracle's incl. two wrong proofs, and the same batch with
    late_rounds = 0 gives the same bytes."""
    from concurrent.futures import ThreadPoolExecutor
    import curdleproofs_amd as cpx
    ell, N = 28, 2048
    crs = orc.generate_crs_points(ell)
    with ThreadPoolExecutor(min(len(os.sched_getaffinity(0)), 64)) as ex:
        insts = list(ex.map(lambda s: orc.make_instance(ell, 70000 + s, crs), range(N)))
    cat = lambda key: b"".join(i[key] for i in insts)
    perms = [x for i in insts for x in i["permutation"]]
    out = {}
    for late in (4, 0):
        c = cpx.Context(0, options={"late_rounds": late})
        try:
            c.set_crs(ell, crs)
            c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
            c.set_profiling(True)
            proofs = c.prove_batch(perms, cat("k"), cat("vec_m_blinders"), cat("prover_rand"))
            assert (c.stat("k_late_msm")["launches"] > 0) == (late == 4) and (c.stat("k_late_uniform")["launches"] > 0) == (late == 4)
            out[late] = proofs
            if late == 4:
                wrong = [j for j, (i, p) in enumerate(zip(insts, proofs)) if p != i["proof"]]
                assert not wrong, "%d proofs differ from the oracle's, first at %d" % (len(wrong), wrong[0])
                bad = list(proofs)
                bad[7], bad[N - 1] = proofs[8], proofs[N - 1][:48 * 3] + proofs[N - 1][48 * 4:48 * 5] + proofs[N - 1][48 * 3:48 * 4] + proofs[N - 1][48 * 5:]
                got = c.verify_batch(bad, cat("verifier_rand"))
                assert [j for j in range(N) if got[j] != cpx.CPX_OK] == [7, N - 1] and got[7] == got[N - 1] == cpx.CPX_ERR_VERIFY
        finally:
            c.close()
    assert out[4] == out[0]


def test_options_are_per_context_and_validated(ctx):
    """cpx_ctx_set_option: unknown keys and out-of-range values are argument errors; an option set on one context does not leak
    into another one (the environment only seeds the defaults)."""
    import curdleproofs_amd as cpx
    other = cpx.Context(0)
    try:
        before = ctx.get_option("device_min_batch")
        other.set_option("device_min_batch", before + 5)
        assert ctx.get_option("device_min_batch") == before and other.get_option("device_min_batch") == before + 5
        for key, value in (("no_such_option", 1), ("fix_bits", 12), ("tbw_wpw", 3), ("tbw_slices", 3), ("device_min_batch", 0)):
            with pytest.raises(cpx.CpxError) as e:
                other.set_option(key, value)
            assert e.value.code == cpx.CPX_ERR_ARG
        with pytest.raises(cpx.CpxError):   # a bad option at construction: the error surfaces and the native context is released again
            cpx.Context(0, options={"no_such_option": 1})
    finally:
        other.close()


def _proof_offsets(ell):
    """byte offsets inside CurdleproofsProof::serialize (curdleproofs.rs:300-310 and the sub-proofs' serialisers)"""
    L = (ell + 4).bit_length() - 1
    o = 9 * 48                   # A cm_T(2) cm_U(2) R S | B | C
    off = {"A": 0, "cm_T_T1": 48, "cm_T_T2": 96, "cm_U_T1": 144, "cm_U_T2": 192, "R": 240, "S": 288, "B": 336, "C": 384, "r_p": o}
    off["B_c"], off["B_d"] = o + 32, o + 80
    off["L_C"], off["R_C"], off["L_D"], off["R_D"] = (o + 128 + q * L * 48 for q in range(4))
    o += 32 + (2 + 4 * L) * 48   # B_c B_d L_C R_C L_D R_D
    off["c"], off["d"] = o, o + 32
    o += 64
    off["cm_A_T1"], off["cm_A_T2"], off["cm_B_T1"], off["cm_B_T2"] = o, o + 48, o + 96, o + 144
    o += 4 * 48
    off["z_k"], off["z_t"], off["z_u"] = o, o + 32, o + 64
    off["B_a"], off["B_t"], off["B_u"] = o + 96, o + 144, o + 192
    off["L_A"], off["L_T"], off["L_U"] = (o + 96 + (3 + q * L) * 48 for q in range(3))
    off["R_A"], off["R_T"], off["R_U"] = (o + 96 + (3 + (3 + q) * L) * 48 for q in range(3))
    o += 96 + (3 + 6 * L) * 48
    off["x"] = o
    assert o + 32 == 48 * (18 + 10 * L) + 32 * 7
    return off


@pytest.fixture(params=["host_driven", "device_resident"])
def path_ctx(request, ctx):
    """a context on which a batch of four proofs takes the named verifier path: the module's context at its default options (the
    host drives the transcripts below `device_min_batch` proofs), or one with that option lowered (everything on the GPU)"""
    import curdleproofs_amd as cpx
    if request.param == "host_driven":
        assert ctx.get_option("device_min_batch") > 4
        yield ctx
    else:
        c = cpx.Context(0, options={"device_min_batch": 1})
        yield c
        c.close()


def test_fused_partial_sums_agree_between_the_verifier_paths(ctx, orc):
    """The table of the accumulated check's weights (csrc/check_weights.hpp) as both verifier paths apply it.  The partial sum of a
    fused batch that holds wrong proofs is sum_i weight_i . point_i != O and depends on every weight, so the same batch with the same
    twelve factors per proof must give the same point on the host-driven path and on the device-resident one."""
    import curdleproofs_amd as cpx
    ell = 28
    crs = orc.generate_crs_points(ell)
    insts = [orc.make_instance(ell, s, crs) for s in (21, 22, 23, 24)]
    cat = lambda key: b"".join(i[key] for i in insts)
    frand = orc.rng(919).fr(12 * len(insts))
    identity = bytes([0xc0]) + bytes(47)
    proofs = [i["proof"] for i in insts]
    off = _proof_offsets(ell)
    rng = orc.rng(929)
    wrong = list(proofs)
    for victim, field, repl in ((1, "z_t", orc.fr_to_canonical_bytes(rng.fr(1))), (3, "L_T", orc.g1_compress(rng.g1_affine(1)))):
        bad = bytearray(wrong[victim])
        bad[off[field]:off[field] + len(repl)] = repl
        wrong[victim] = bytes(bad)
        x = insts[victim]
        assert orc.verify(ell, crs, x["vec_R"], x["vec_S"], x["vec_T"], x["vec_U"], x["M"], wrong[victim], x["verifier_rand"]) == 0, field
    assert ctx.get_option("device_min_batch") > len(insts)
    dev = cpx.Context(0, options={"device_min_batch": 1})
    try:
        sums = []
        for c in (ctx, dev):
            c.set_crs(ell, crs)
            c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
            part, nbad = c.verify_batch_fused_partial(proofs, frand)
            assert nbad == 0 and orc.g1_compress_jac(part) == identity
            part, nbad = c.verify_batch_fused_partial(wrong, frand)
            assert nbad == 0
            sums.append(orc.g1_compress_jac(part))
        assert sums[0] == sums[1]
        assert sums[0] != identity
    finally:
        dev.close()


def test_same_scalar_relations_are_checked(path_ctx, orc):
    """same_scalar_argument.rs:96-137.  z_k, z_t, z_u are never absorbed into the transcript, so re-encoding a proof with
    one of them replaced by another canonical scalar breaks ONLY the SameScalar equalities (every challenge and every other
    check stays as it was): the verdict must be VerificationError, as the oracle's.  Same for cm_A.T_1 / cm_B.T_2 replaced
    by another valid point.  Both verifier forms (per proof, fused) and a fused batch with exactly one such proof, on the host-driven
    and on the device-resident path."""
    import curdleproofs_amd as cpx
    ctx = path_ctx
    ell = 28
    seeds = [11, 12, 13, 14]
    crs = orc.generate_crs_points(ell)
    ctx.set_crs(ell, crs)
    insts = [orc.make_instance(ell, s, crs) for s in seeds]
    cat = lambda key: b"".join(i[key] for i in insts)
    ctx.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
    proofs = [i["proof"] for i in insts]
    vrand = cat("verifier_rand")
    frand = orc.rng(515).fr(12 * len(seeds))
    assert ctx.verify_batch(proofs, vrand) == [cpx.CPX_OK] * 4
    assert ctx.verify_batch_fused(proofs, frand)
    off = _proof_offsets(ell)
    rng = orc.rng(616)
    other_scalar = orc.fr_to_canonical_bytes(rng.fr(1))
    other_point = orc.g1_compress(rng.g1_affine(1))

    def oracle_verdict(i, proof):
        x = insts[i]
        return orc.verify(ell, crs, x["vec_R"], x["vec_S"], x["vec_T"], x["vec_U"], x["M"], proof, x["verifier_rand"])

    for field, repl in [("z_k", other_scalar), ("z_t", other_scalar), ("z_u", other_scalar), ("cm_A_T1", other_point), ("cm_B_T2", other_point)]:
        for victim in (0, 2):
            bad = bytearray(proofs[victim])
            bad[off[field]:off[field] + len(repl)] = repl
            bad = bytes(bad)
            assert oracle_verdict(victim, bad) == 0, field
            mixed = list(proofs)
            mixed[victim] = bad
            want = [cpx.CPX_OK] * 4
            want[victim] = cpx.CPX_ERR_VERIFY
            assert ctx.verify_batch(mixed, vrand) == want, field
            assert not ctx.verify_batch_fused(mixed, frand), field
            part, nbad = ctx.verify_batch_fused_partial(mixed, frand)
            assert nbad == 0 and orc.g1_compress_jac(part)[0] != 0xC0, field
    # z_k + 1 (a "nearby" scalar, still canonical)
    zk = int.from_bytes(proofs[1][off["z_k"]:off["z_k"] + 32], "little")
    bad = bytearray(proofs[1])
    bad[off["z_k"]:off["z_k"] + 32] = ((zk + 1) % 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001).to_bytes(32, "little")
    assert oracle_verdict(1, bytes(bad)) == 0
    assert ctx.verify_batch([proofs[0], bytes(bad), proofs[2], proofs[3]], vrand) == [cpx.CPX_OK, cpx.CPX_ERR_VERIFY, cpx.CPX_OK, cpx.CPX_OK]


@pytest.mark.parametrize("copies", [1, 97], ids=["host_driven", "device_resident"])
def test_single_field_negatives_of_every_sub_argument(ctx, orc, copies):
    """The reference's sub-argument negatives — a wrong inner product (inner_product_argument.rs:432-446), a wrong grand product
    and a wrong `B` (grand_product_argument.rs:316-373) — at the level this boundary sees them: ONE field of a valid serialized proof
    replaced by another valid encoding (a canonical scalar / a subgroup point), everything else untouched.  r_p (GrandProduct), c, d
    (IPA), x (SameMSM), z_k (SameScalar), and one point of every sub-proof: B (SamePerm), C (GrandProduct), B_c, L_C[1], R_D[0] (IPA),
    cm_A.T_2 (SameScalar), B_a, L_T[0], R_U[last] (SameMSM), A / cm_T.T_1 / R (top level).  Verdicts of the per-proof verifier must equal
    the oracle's (all VerificationError), and the fused verifier must reject a batch holding one such proof — on the host-driven
    path (one proof per call) and the device-resident one (the mutated proof inside a batch of 97)."""
    import curdleproofs_amd as cpx
    ell = 28
    L = 5
    crs = orc.generate_crs_points(ell)
    ctx.set_crs(ell, crs)
    inst = orc.make_instance(ell, 77, crs)
    good = inst["proof"]
    cat = lambda key: inst[key] * copies
    ctx.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
    vrand = inst["verifier_rand"] * copies
    frand = orc.rng(818).fr(12 * copies)
    assert ctx.verify_batch([good] * copies, vrand) == [cpx.CPX_OK] * copies
    assert ctx.verify_batch_fused([good] * copies, frand)
    off = _proof_offsets(ell)
    rng = orc.rng(717)
    scalar = orc.fr_to_canonical_bytes(rng.fr(1))
    point = orc.g1_compress(rng.g1_affine(1))
    fields = [("r_p", 0, scalar), ("c", 0, scalar), ("d", 0, scalar), ("x", 0, scalar), ("z_k", 0, scalar),
              ("A", 0, point), ("cm_T_T1", 0, point), ("R", 0, point), ("B", 0, point), ("C", 0, point), ("B_c", 0, point), ("L_C", 1, point),
              ("R_D", 0, point), ("cm_A_T2", 0, point), ("B_a", 0, point), ("L_T", 0, point), ("R_U", L - 1, point)]
    victim = copies // 2
    for field, j, repl in fields:
        o = off[field] + 48 * j
        assert good[o:o + len(repl)] != repl
        bad = good[:o] + repl + good[o + len(repl):]
        want = orc.verify(ell, crs, inst["vec_R"], inst["vec_S"], inst["vec_T"], inst["vec_U"], inst["M"], bad, inst["verifier_rand"])
        assert want == 0, (field, want)      # the reference's tests expect VerificationError for each of these
        proofs = [good] * copies
        proofs[victim] = bad
        expect = [cpx.CPX_OK] * copies
        expect[victim] = cpx.CPX_ERR_VERIFY
        assert ctx.verify_batch(proofs, vrand) == expect, field
        assert not ctx.verify_batch_fused(proofs, frand), field
    # the identity in place of a proof point is a valid encoding too (curdleproofs.rs:312-323 deserialises it): still a wrong proof
    o = off["L_D"]
    bad = good[:o] + bytes([0xc0]) + bytes(47) + good[o + 48:]
    want = orc.verify(ell, crs, inst["vec_R"], inst["vec_S"], inst["vec_T"], inst["vec_U"], inst["M"], bad, inst["verifier_rand"])
    proofs = [good] * copies
    proofs[victim] = bad
    got = ctx.verify_batch(proofs, vrand)
    assert want == 0 and got[victim] == cpx.CPX_ERR_VERIFY and got.count(cpx.CPX_OK) == copies - 1


def test_crs_switch_at_equal_ell_on_the_device_path(orc):
    """Two different CRS of the same ell on one context, batches large enough for the device-resident protocol: the cached device
    plans embed the compressed H and table addresses of the CRS they were built for, so set_crs must drop them (a new table
    allocation of the same size may land on the same addresses).  Proof bytes and verdicts against the oracle under both CRS,
    in the order first -> second -> first."""
    import curdleproofs_amd as cpx
    ell, nb = 28, 100
    crs_a = orc.generate_crs_points(ell)
    crs_b = orc.rng(31337).g1_affine(ell + 7)
    assert crs_a != crs_b
    c = cpx.Context(0)
    try:
        for crs in (crs_a, crs_b, crs_a):
            c.set_crs(ell, crs)
            insts = [orc.make_instance(ell, 300 + s, crs) for s in range(4)]
            insts = [insts[i % 4] for i in range(nb)]
            cat = lambda key: b"".join(i[key] for i in insts)
            c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
            proofs = c.prove_batch([x for i in insts for x in i["permutation"]], cat("k"), cat("vec_m_blinders"), cat("prover_rand"))
            assert [p == i["proof"] for p, i in zip(proofs, insts)] == [True] * nb
            assert c.verify_batch(proofs, cat("verifier_rand")) == [cpx.CPX_OK] * nb
            assert c.verify_batch_fused(proofs, orc.rng(5).fr(12 * nb))
    finally:
        c.close()


def test_headline_shape_1024_proofs_ell252_every_proof_matches_oracle(orc):
    """BASELINE configs[3] at its literal shape — 1024 independent instances at ell = 252, instance i from StdRng(i) — on ONE GPU the
    way bench.py drives it: two engine contexts x 512 proofs from two host threads at once, default options (k_msm_fix<16, 16>,
    k_msm_tblw<32, false>, the thread-per-group reductions, the device-resident protocol).  EVERY proof must equal the oracle's
    bytes and every verdict the oracle's (three deliberately wrong proofs per context); then configs[4]'s batched verifier over the
    same 1024 proofs: the two contexts' partial sums add up to the identity for the valid batch and do not once wrong proofs are
    in it (curdleproofs.rs:385-471 + msm_accumulator.rs:38-68 at the headline size)."""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    import curdleproofs_amd as cpx
    ell, K, N = 252, 2, 1024
    crs = orc.generate_crs_points(ell)
    insts = _instance_list(orc, ell, N, crs)   # ~0.7 s per instance and core, shared with the one-context test of the bench shape
    assert all(i["verdict"] == 1 for i in insts)
    per = N // K
    errors = []
    partials, partials_bad = [None] * K, [None] * K

    def run(k):
        try:
            c = cpx.Context(0)
            c.set_crs(ell, crs)
            mine = insts[k * per:(k + 1) * per]
            cat = lambda key: b"".join(i[key] for i in mine)
            c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
            proofs = c.prove_batch([x for i in mine for x in i["permutation"]], cat("k"), cat("vec_m_blinders"), cat("prover_rand"))
            wrong = [j for j, (i, p) in enumerate(zip(mine, proofs)) if p != i["proof"]]
            if wrong:
                errors.append("context %d: %d of %d proofs differ from the oracle's, first at index %d" % (k, len(wrong), per, wrong[0]))
            good = [i["proof"] for i in mine]
            bad = list(good)
            bad[5] = good[6]                                                        # a neighbour's proof
            bad[per // 2] = good[per // 2][48:96] + good[per // 2][:48] + good[per // 2][96:]   # two points swapped
            last = bytearray(good[per - 1])
            last[-1] ^= 0x01                                                        # the last scalar changed
            bad[per - 1] = bytes(last)
            got = c.verify_batch(bad, cat("verifier_rand"))
            want = [cpx.CPX_OK] * per
            for j in (5, per // 2, per - 1):
                x = mine[j]
                o = orc.verify(ell, crs, x["vec_R"], x["vec_S"], x["vec_T"], x["vec_U"], x["M"], bad[j], x["verifier_rand"])
                want[j] = {1: cpx.CPX_OK, 0: cpx.CPX_ERR_VERIFY, -1: cpx.CPX_ERR_DESERIALIZE}[o]
            if got != want:
                errors.append("context %d: verdicts differ at %s" % (k, [j for j in range(per) if got[j] != want[j]][:8]))
            if c.verify_batch(good, cat("verifier_rand")) != [cpx.CPX_OK] * per:
                errors.append("context %d: a valid proof was rejected" % k)
            frand = orc.rng(9100 + k).fr(12 * per)
            partials[k] = c.verify_batch_fused_partial(good, frand)
            partials_bad[k] = c.verify_batch_fused_partial(bad, frand) if k == 1 else partials[k]
            c.close()
        except Exception as e:   # surfaced below
            errors.append("context %d: %r" % (k, e))

    th = [threading.Thread(target=run, args=(k,)) for k in range(K)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    c = cpx.Context(0)
    assert all(b == 0 for _, b in partials)
    assert c.sum_jac(b"".join(p for p, _ in partials))[1], "partial sums of 1024 valid ell=252 proofs must add up to the identity"
    assert not c.sum_jac(b"".join(p for p, _ in partials_bad))[1]
    c.close()


_INSTANCE_LISTS = {}


_DISTINCT = {252: 1024, 1020: 128}   # distinct oracle instances per proof size the large shapes draw from (the rest of a batch repeats them)


def _instance_list(orc, ell, count, crs):
    """`count` instances of BASELINE configs[3]'s recipe (instance i from StdRng(i mod D)), computed once per session on all host cores (the
    oracle is a C library behind ctypes: the GIL is released) and shared by the tests of the large shapes.  D distinct instances (1024 at
    ell = 252 — BASELINE configs[3]'s own count —, 128 at ell = 1020), repeated beyond that: the oracle needs 0.9 / 3.2 s per instance and
    core, and the GPU suite has to stay well inside the driver's time limit (round 5: 2048 + 512 distinct ones were 250 s of a 634-s suite)."""
    from concurrent.futures import ThreadPoolExecutor
    have = _INSTANCE_LISTS.setdefault(ell, [])
    want = min(count, _DISTINCT.get(ell, count))
    if len(have) < want:
        ncpu = min(len(os.sched_getaffinity(0)), os.cpu_count() or 8, 64)
        with ThreadPoolExecutor(ncpu) as ex:
            have.extend(ex.map(lambda s: orc._make_instance(ell, s, crs), range(len(have), want)))
    return [have[i % want] for i in range(count)]


def _three_wrong(good):
    """a neighbour's proof, two points swapped, the last scalar changed"""
    per = len(good)
    bad = list(good)
    bad[5] = good[6]
    bad[per // 2] = good[per // 2][48:96] + good[per // 2][:48] + good[per // 2][96:]
    last = bytearray(good[per - 1])
    last[-1] ^= 0x01
    bad[per - 1] = bytes(last)
    return bad, (5, per // 2, per - 1)


@pytest.mark.parametrize("ell,N", [(252, 2048), (1020, 512)], ids=["bench_shape_2048_x_ell252", "bench_shape_512_x_ell1020"])
def test_bench_code_path_one_context_default_options_every_proof_matches_oracle(orc, ell, N):
    """The configuration that produces the bench numbers, pinned on EVERY proof: one engine context with DEFAULT options (but for the batch
    size from which the one-lane transcript kernel takes over, see below) holding a batch
    large enough for the late rounds on materialised folded bases (late.hip: >= 2048 proofs at ell = 252 — the bench runs 8192 per
    context —, >= 512 at ell = 1020 — the `ell_1020` key runs 2048), i.e. k_msm_fix<16, 16>, k_msm_tblw<32, false>, the thread-per-group
    reductions, k_late_fix / k_late_uniform / k_late_tables / k_late_msm and the device-resident protocol all at once.  Every proof's
    bytes and every verdict (three deliberately wrong proofs) must equal the oracle's, then BASELINE configs[4]'s fused verifier over
    the same batch (curdleproofs.rs:385-471, inner_product_argument.rs:150-186, same_multiscalar_argument.rs:99-136)."""
    import curdleproofs_amd as cpx
    crs = orc.generate_crs_points(ell)
    insts = _instance_list(orc, ell, N, crs)
    assert all(i["verdict"] == 1 for i in insts)
    cat = lambda key: b"".join(i[key] for i in insts)
    c = cpx.Context(0)
    try:
        assert c.get_option("late_rounds") == 4 and c.get_option("fix_bits") == 16 and c.get_option("transcript_lane_min_batch") == 8192
        if ell == 252:   # the ONE option that differs from the defaults: the bench's contexts hold 8192 proofs and therefore hash the transcript
            c.set_option("transcript_lane_min_batch", N)   # prefix with k_transcript_step1_lane; 2048 proofs only reach it with the threshold lowered
        c.set_crs(ell, crs)
        if c.get_option("fix_bits_effective") != 16:
            pytest.skip("not enough free HBM for the 16-bit fixed-base table at ell = %d (other contexts' tables resident): the bench shape cannot run here" % ell)
        c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
        c.set_profiling(True)
        c.reset_stats()
        proofs = c.prove_batch([x for i in insts for x in i["permutation"]], cat("k"), cat("vec_m_blinders"), cat("prover_rand"))
        for name in ("k_late_fix", "k_late_uniform", "k_late_tables", "k_late_msm", "k_msm_fix<16, 16>", "k_msm_tblw<32, false>", "k_transcript_step1"):
            assert c.stat(name)["launches"] > 0, "%s did not run: this is not the bench's code path" % name
        c.set_profiling(False)
        wrong = [j for j, (i, p) in enumerate(zip(insts, proofs)) if p != i["proof"]]
        assert not wrong, "%d of %d proofs differ from the oracle's, first at index %d" % (len(wrong), N, wrong[0])
        good = [i["proof"] for i in insts]
        bad, where = _three_wrong(good)
        got = c.verify_batch(bad, cat("verifier_rand"))
        want = [cpx.CPX_OK] * N
        for j in where:
            x = insts[j]
            o = orc.verify(ell, crs, x["vec_R"], x["vec_S"], x["vec_T"], x["vec_U"], x["M"], bad[j], x["verifier_rand"])
            want[j] = {1: cpx.CPX_OK, 0: cpx.CPX_ERR_VERIFY, -1: cpx.CPX_ERR_DESERIALIZE}[o]
        assert all(want[j] != cpx.CPX_OK for j in where)
        assert got == want, "verdicts differ at %s" % [j for j in range(N) if got[j] != want[j]][:8]
        assert c.verify_batch(good, cat("verifier_rand")) == [cpx.CPX_OK] * N
        frand = orc.rng(9300 + ell).fr(12 * N)
        assert c.verify_batch_fused(good, frand)
        assert not c.verify_batch_fused(bad, frand)
    finally:
        c.close()


def test_bench_batch_8192_on_one_context_and_config5_literal_4096_in_one_check(orc):
    """(1) The headline's per-context shape with NOTHING lowered: 8192 ell = 252 proofs on ONE engine context with default options — the
    one-lane transcript prefix (k_transcript_step1_lane takes over at 8192), the late rounds, k_msm_fix<16, 16>, k_msm_tblw<32, false> at
    the grid sizes the bench launches.  The batch is instances 0..2047 of BASELINE configs[3]'s recipe four times over (instance j mod 2048
    in place j: the oracle's proof of every place is known), and EVERY proof is compared with the oracle's bytes — the random sample of
    64 the review asked for is a subset.  (2) BASELINE configs[4] at its literal size: the first 4096 of those proofs in ONE accumulated
    check (msm_accumulator.rs:55-68 shared by all verify calls) with fresh factors — accepted; with one proof replaced by a neighbour's
    (a valid proof of another instance) — refused; and the per-proof verifier's verdicts on the same 4096."""
    import random
    import curdleproofs_amd as cpx
    ell, D, N, NF = 252, 2048, 8192, 4096
    crs = orc.generate_crs_points(ell)
    insts = _instance_list(orc, ell, D, crs)
    rep = N // D
    cat = lambda key: b"".join(i[key] for i in insts) * rep
    c = cpx.Context(0)
    try:
        assert c.get_option("transcript_lane_min_batch") == 8192 and c.get_option("late_rounds") == 4 and c.get_option("fix_bits") == 16
        c.set_crs(ell, crs)
        if c.get_option("fix_bits_effective") != 16:
            pytest.skip("not enough free HBM for the 16-bit fixed-base table")
        c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
        c.set_profiling(True)
        c.reset_stats()
        proofs = c.prove_batch([x for i in insts for x in i["permutation"]] * rep, cat("k"), cat("vec_m_blinders"), cat("prover_rand"))
        for name in ("k_late_msm", "k_msm_fix<16, 16>", "k_msm_tblw<32, false>", "k_transcript_step1"):
            assert c.stat(name)["launches"] > 0, "%s did not run" % name
        c.set_profiling(False)
        wrong = [j for j in range(N) if proofs[j] != insts[j % D]["proof"]]
        assert not wrong, "%d of %d proofs differ from the oracle's, first at place %d" % (len(wrong), N, wrong[0])
        sample = random.Random(5).sample(range(N), 64)
        assert all(proofs[j] == insts[j % D]["proof"] for j in sample)
        assert c.verify_batch(proofs, cat("verifier_rand")) == [cpx.CPX_OK] * N
        # config 5, literally: 4096 proofs, one accumulated check
        cut = lambda key: b"".join(i[key] for i in insts) * (NF // D)
        c.load_batch(cut("vec_R"), cut("vec_S"), cut("vec_T"), cut("vec_U"), cut("M"))
        good = proofs[:NF]
        frand = orc.rng(9401).fr(12 * NF)
        assert c.verify_batch_fused(good, frand)
        bad = list(good)
        bad[3000] = good[3001]
        assert not c.verify_batch_fused(bad, frand)
        assert c.verify_batch_fused(good, orc.rng(9402).fr(12 * NF))          # fresh factors, same verdict
        got = c.verify_batch(bad, cut("verifier_rand"))
        x = insts[3000 % D]
        assert orc.verify(ell, crs, x["vec_R"], x["vec_S"], x["vec_T"], x["vec_U"], x["M"], bad[3000], x["verifier_rand"]) == 0
        assert got == [cpx.CPX_OK] * 3000 + [cpx.CPX_ERR_VERIFY] + [cpx.CPX_OK] * (NF - 3001)
    finally:
        c.close()


def test_verifier_rejects_degenerate_random_factors(ctx, orc):
    """include/cpx.h: the accumulate_check factors must be uniform non-zero field elements (msm_accumulator.rs:44 draws
    Fr::rand); a zero or non-reduced factor would silently drop a check, so it is an argument error."""
    import curdleproofs_amd as cpx
    ell = 28
    crs = orc.generate_crs_points(ell)
    ctx.set_crs(ell, crs)
    inst = orc.make_instance(ell, 21, crs)
    ctx.load_batch(inst["vec_R"], inst["vec_S"], inst["vec_T"], inst["vec_U"], inst["M"])
    vr = bytearray(inst["verifier_rand"])
    for repl in (bytes(32), b"\xff" * 32):
        for slot in (0, 5):
            bad = bytearray(vr)
            bad[32 * slot:32 * slot + 32] = repl
            with pytest.raises(cpx.CpxError) as e:
                ctx.verify_batch([inst["proof"]], bytes(bad))
            assert e.value.code == cpx.CPX_ERR_ARG
    fr = bytearray(orc.rng(1).fr(12))
    fr[32 * 9:32 * 10] = bytes(32)
    with pytest.raises(cpx.CpxError) as e:
        ctx.verify_batch_fused_partial([inst["proof"]], bytes(fr))
    assert e.value.code == cpx.CPX_ERR_ARG
    assert ctx.verify_batch([inst["proof"]], bytes(vr)) == [cpx.CPX_OK]


def test_large_batch_four_contexts_every_proof_matches_oracle(orc):
    """BASELINE config 4 recipe at oracle-friendly size: >= 1024 independent instances (instance i from StdRng(i)) split over
    FOUR engine contexts driven by four host threads at once (the bench's mode of operation: shared CRS tables, concurrent
    streams, worker pools side by side).  EVERY proof must equal the oracle's bytes and every verdict the oracle's,
    including a few deliberately wrong proofs per context."""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    import curdleproofs_amd as cpx
    ell, K = 28, 4
    ncpu = os.cpu_count() or 8
    N = 2048 if ncpu >= 32 else 1024     # 512 proofs per context: P1 alone has 4608 fixed-base tasks -> k_msm_fix<16, 16>
    crs = orc.generate_crs_points(ell)
    with ThreadPoolExecutor(min(ncpu, 64)) as ex:   # the oracle is a C library behind ctypes: the threads run in parallel
        insts = list(ex.map(lambda s: orc.make_instance(ell, 5000 + s, crs), range(N)))
    per = N // K
    errors = []
    partials, partials_bad = [None] * K, [None] * K

    def run(k):
        try:
            c = cpx.Context(0)
            c.set_crs(ell, crs)
            mine = insts[k * per:(k + 1) * per]
            cat = lambda key: b"".join(i[key] for i in mine)
            c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
            proofs = c.prove_batch([x for i in mine for x in i["permutation"]], cat("k"), cat("vec_m_blinders"), cat("prover_rand"))
            wrong = [j for j, (i, p) in enumerate(zip(mine, proofs)) if p != i["proof"]]
            if wrong:
                errors.append("context %d: %d proofs differ from the oracle's, first at index %d" % (k, len(wrong), wrong[0]))
            # verdicts: three wrong proofs per context (a neighbour's proof; swapped points; a flipped scalar)
            proofs = list(proofs)
            proofs[3] = proofs[4]
            proofs[per // 2] = proofs[per // 2][48:96] + proofs[per // 2][:48] + proofs[per // 2][96:]
            last = bytearray(proofs[per - 1])
            last[-1] ^= 0x01
            proofs[per - 1] = bytes(last)
            got = c.verify_batch(proofs, cat("verifier_rand"))
            want = [cpx.CPX_OK] * per
            for j in (3, per // 2, per - 1):
                x = mine[j]
                o = orc.verify(ell, crs, x["vec_R"], x["vec_S"], x["vec_T"], x["vec_U"], x["M"], proofs[j], x["verifier_rand"])
                want[j] = {1: cpx.CPX_OK, 0: cpx.CPX_ERR_VERIFY, -1: cpx.CPX_ERR_DESERIALIZE}[o]
            if got != want:
                errors.append("context %d: verdicts differ at %s" % (k, [j for j in range(per) if got[j] != want[j]][:8]))
            # BASELINE config 5 at this scale: the context's share of ONE accumulated check over all N proofs (12 factors per proof);
            # the four partial sums are added below like the all-gather step does
            frand = orc.rng(9000 + k).fr(12 * per)
            good = [i["proof"] for i in mine]
            partials[k] = c.verify_batch_fused_partial(good, frand)
            partials_bad[k] = c.verify_batch_fused_partial(proofs, frand) if k == 2 else partials[k]   # context 2 holds three wrong proofs
            c.close()
        except Exception as e:   # surfaced below (an exception in a thread would otherwise be lost)
            errors.append("context %d: %r" % (k, e))

    th = [threading.Thread(target=run, args=(k,)) for k in range(K)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    c = cpx.Context(0)
    assert all(b == 0 for _, b in partials)
    assert c.sum_jac(b"".join(p for p, _ in partials))[1], "the partial sums of %d valid proofs on four contexts must add up to the identity" % N
    assert not c.sum_jac(b"".join(p for p, _ in partials_bad))[1]


RCCL_WORKER = r"""
import os, sys, json
sys.path.insert(0, %r)
import torch, torch.distributed as dist
import curdleproofs_amd as cpx
from curdleproofs_amd.dist import max_over_ranks, all_gather_partials, fused_verify_all_ranks, partition
from tests.oracle_lib import Oracle
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(rank)
dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))   # nccl == RCCL on ROCm
orc = Oracle()
ell = 28
crs = orc.generate_crs_points(ell)
every = [orc.make_instance(ell, 40 + s, crs) for s in range(3 * world)]
insts = [every[i] for i in partition(len(every), world, rank)]       # this rank's share of ONE accumulated check over all proofs
cat = lambda key: b"".join(i[key] for i in insts)
c = cpx.Context(rank)                                                 # one context per GPU: rank r drives device r
c.set_crs(ell, crs)
c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
proofs = [i["proof"] for i in insts]
rand = orc.rng(3 + rank).fr(12 * len(insts))
dist.barrier()
tmax = max_over_ranks(1.25 + rank, dist, "cuda")               # ncclAllReduce(MAX) on a device tensor: the bench's timing step
part, bad = c.verify_batch_fused_partial(proofs, rand)
parts, bad_total = all_gather_partials(part, bad, dist, "cuda")   # ncclAllGather of the 148-byte payload on device tensors
ok = fused_verify_all_ranks(c, proofs, rand, dist, "cuda")
swapped = [proofs[1], proofs[0], proofs[2]] if rank == world - 1 else proofs   # ONE rank holds wrong proofs: every rank must refuse
wrong = fused_verify_all_ranks(c, swapped, rand, dist, "cuda")
if rank == 0:
    print(json.dumps(dict(backend=dist.get_backend(), world=world, tmax=tmax, nparts=len(parts) // 144, mine_first=parts[:144] == part, bad=bad_total, ok=bool(ok),
                          wrong=bool(wrong), all_identity=c.sum_jac(parts)[1])))
dist.barrier()
dist.destroy_process_group()
"""


def test_rccl_collectives_of_the_fused_verifier_run_on_the_gpu(tmp_path):
    """The exchange step of BASELINE configs[4] and the bench's timing reduction through backend "nccl" (= RCCL) on device tensors, with
    world = min(2, visible GPUs) ranks, rank r on device r.  On a 1-GPU box the communicator has ONE rank (RCCL refuses two ranks on
    one device): the same ncclAllGather / ncclAllReduce calls on the same tensors; with a second GPU present the partial sums really
    cross xGMI, one rank holds the wrong proofs and every rank must refuse the batch.  (The N = 2 data flow is also covered over gloo:
    tests/test_distributed_cpu.py and test_bench_two_ranks_on_one_gpu.)"""
    import json
    import subprocess
    import sys
    import curdleproofs_amd as cpx
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    world = min(2, cpx.device_count())
    script = tmp_path / "rccl_worker.py"
    script.write_text(RCCL_WORKER % root)
    procs = []
    for rank in range(world):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29641", RANK=str(rank), WORLD_SIZE=str(world),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        env.pop("LOCAL_RANK", None)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=900) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, o[-1500:] + e[-3000:]
    d = json.loads([l for l in outs[0][0].splitlines() if l.startswith("{")][-1])
    assert d == dict(backend="nccl", world=world, tmax=1.25 + world - 1, nparts=world, mine_first=True, bad=0, ok=True, wrong=False, all_identity=True)


def _multi_device_shares(orc, ell, per_dev, ndev):
    crs = orc.generate_crs_points(ell)
    insts = [orc.make_instance(ell, 8000 + s, crs) for s in range(per_dev * ndev)]
    return crs, [insts[d * per_dev:(d + 1) * per_dev] for d in range(ndev)]


@pytest.mark.parametrize("ndev", [1, 2, 8], ids=["one_gpu", "two_gpus", "eight_gpus"])
def test_configs_4_and_5_in_process_over_the_visible_devices(orc, ndev):
    """BASELINE configs[3] / configs[4] the way a Rust caller of the C-ABI would run them on a multi-GPU node, WITHOUT torch or RCCL: one
    engine context and one host thread per device (cpx_ctx_create(d)), independent proofs sharded over the devices (no collective:
    msm_accumulator.rs:55-68 needs none for per-proof verification), and for the batched verifier every device's 144-byte partial sum
    (cpx_batch_verify_fused) brought to ONE context and added with cpx_g1_sum_jac — the in-process equivalent of the all-gather.
    Runs on min(ndev, visible) ... skipped when the box has fewer than ndev GPUs (1-GPU boxes run the first case only)."""
    import threading
    import curdleproofs_amd as cpx
    if cpx.device_count() < ndev:
        pytest.skip("needs %d GPUs, %d visible" % (ndev, cpx.device_count()))
    ell, per_dev = 28, 100   # >= 56 proofs per device: the device-resident protocol
    crs, shares = _multi_device_shares(orc, ell, 4, ndev)
    shares = [[sh[i % len(sh)] for i in range(per_dev)] for sh in shares]
    partials, partials_bad, errors = [None] * ndev, [None] * ndev, []

    def run(d):
        try:
            c = cpx.Context(d)
            mine = shares[d]
            cat = lambda key: b"".join(i[key] for i in mine)
            c.set_crs(ell, crs)
            c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
            proofs = c.prove_batch([x for i in mine for x in i["permutation"]], cat("k"), cat("vec_m_blinders"), cat("prover_rand"))
            if [p == i["proof"] for p, i in zip(proofs, mine)] != [True] * per_dev:
                errors.append("device %d: proof bytes differ from the oracle's" % d)
            if c.verify_batch(proofs, cat("verifier_rand")) != [cpx.CPX_OK] * per_dev:
                errors.append("device %d: a valid proof was rejected" % d)
            frand = orc.rng(700 + d).fr(12 * per_dev)
            partials[d] = c.verify_batch_fused_partial(proofs, frand)
            bad = list(proofs)
            bad[3] = proofs[2] if proofs[2] != proofs[3] else proofs[1]
            partials_bad[d] = c.verify_batch_fused_partial(bad, frand) if d == ndev - 1 else partials[d]
            c.close()
        except Exception as e:
            errors.append("device %d: %r" % (d, e))

    th = [threading.Thread(target=run, args=(d,)) for d in range(ndev)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    c0 = cpx.Context(0)
    try:
        assert all(b == 0 for _, b in partials)
        assert c0.sum_jac(b"".join(p for p, _ in partials))[1], "the partial sums of all devices must add up to the identity"
        assert not c0.sum_jac(b"".join(p for p, _ in partials_bad))[1], "one device holds a wrong proof: the batch must be refused"
    finally:
        c0.close()


def test_four_contexts_switching_crs_concurrently_stay_bit_exact(orc):
    """Engine robustness (the sanitizer runs cover the host headers, not engine.cpp): FOUR contexts on four host threads, each walking its
    own sequence over four CRS — two different CRS at ell = 28 and two at ell = 60 — with batches of 96 (device-resident protocol, cached
    plans) in between: the process-wide registry of shared CRS tables (engine.cpp set_crs_impl: weak pointers, tables built once per
    (device, CRS), released with their last context) and every context's plan caches are exercised CONCURRENTLY — contexts asking for
    the same table at the same time, a table released by one context while another still proves with it, a context coming back to a
    CRS whose table has meanwhile been rebuilt at another address.  Every proof's bytes and every verdict equal the oracle's."""
    import threading
    import curdleproofs_amd as cpx
    nb = 96
    crs_sets = {}
    for ell in (28, 60):
        for tag, pts in (("a", orc.generate_crs_points(ell)), ("b", orc.rng(4000 + ell).g1_affine(ell + 7))):
            insts = [orc.make_instance(ell, 600 + s, pts) for s in range(3)]
            crs_sets[(ell, tag)] = (pts, [insts[i % 3] for i in range(nb)])
    keys = sorted(crs_sets)
    errors = []

    def run(t):
        try:
            c = cpx.Context(0)
            order = [keys[(t + j * (1 + t % 3)) % 4] for j in range(6)]   # every thread its own walk; neighbours collide on the same CRS
            for key in order:
                ell = key[0]
                pts, insts = crs_sets[key]
                cat = lambda k_: b"".join(i[k_] for i in insts)
                c.set_crs(ell, pts)
                c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
                proofs = c.prove_batch([x for i in insts for x in i["permutation"]], cat("k"), cat("vec_m_blinders"), cat("prover_rand"))
                if [p == i["proof"] for p, i in zip(proofs, insts)] != [True] * nb:
                    errors.append("thread %d, CRS %s: proof bytes differ from the oracle's" % (t, key))
                bad = list(proofs)
                bad[7] = proofs[8]   # instance 8 != instance 7 (three instances repeating)
                got = c.verify_batch(bad, cat("verifier_rand"))
                if got != [cpx.CPX_OK] * 7 + [cpx.CPX_ERR_VERIFY] + [cpx.CPX_OK] * (nb - 8):
                    errors.append("thread %d, CRS %s: verdicts %s" % (t, key, [j for j, v in enumerate(got) if v != cpx.CPX_OK]))
                if not c.verify_batch_fused(proofs, orc.rng(t).fr(12 * nb)):
                    errors.append("thread %d, CRS %s: fused verifier refused a valid batch" % (t, key))
            c.close()
        except Exception as e:
            errors.append("thread %d: %r" % (t, e))

    th = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_small_batch_beside_a_gpu_filling_batch_on_another_context(orc):
    """The prefix and the T_2 scalar multiplications of a batch of <= 256 proofs run in waves that claim a whole SIMD
    (k_transcript_step1<true>, k_smul<true>): such a wave is only placed on a SIMD with no resident wave.  Beside ANOTHER context that
    keeps the GPU full the small batch must still make progress (its work-groups get in whenever SIMDs drain) and stay bit-exact: one
    thread proves / verifies 4096-proof batches in a loop while a second one runs 128-proof passes on its own context, every proof
    and verdict of both against the oracle.  A hang here is a failure (pytest-timeout / the driver's limit)."""
    import threading
    import time
    import curdleproofs_amd as cpx
    ell = 28
    pts = orc.generate_crs_points(ell)
    base = [orc.make_instance(ell, 900 + s, pts) for s in range(4)]
    errors, stop, small_passes = [], threading.Event(), []

    def run(nb, passes, tag):
        try:
            insts = [base[i % 4] for i in range(nb)]
            cat = lambda k_: b"".join(i[k_] for i in insts)
            c = cpx.Context(0)
            c.set_crs(ell, pts)
            c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
            perm = [x for i in insts for x in i["permutation"]]
            args = (perm, cat("k"), cat("vec_m_blinders"), cat("prover_rand"))
            n = 0
            while (passes is None and not stop.is_set()) or (passes is not None and n < passes):
                t0 = time.perf_counter()
                proofs = c.prove_batch(*args)
                if [p == i["proof"] for p, i in zip(proofs, insts)] != [True] * nb:
                    errors.append("%s: proof bytes differ from the oracle's" % tag)
                bad = list(proofs)
                bad[5] = proofs[6]
                got = c.verify_batch(bad, cat("verifier_rand"))
                if got != [cpx.CPX_OK] * 5 + [cpx.CPX_ERR_VERIFY] + [cpx.CPX_OK] * (nb - 6):
                    errors.append("%s: verdicts %s" % (tag, [j for j, v in enumerate(got) if v != cpx.CPX_OK]))
                if passes is not None:
                    small_passes.append(time.perf_counter() - t0)
                n += 1
            c.close()
        except Exception as e:
            errors.append("%s: %r" % (tag, e))

    big = threading.Thread(target=run, args=(4096, None, "4096-proof context"))
    big.start()
    time.sleep(1.0)   # the large context is in its loop
    small = threading.Thread(target=run, args=(128, 12, "128-proof context"))
    small.start()
    small.join(timeout=600)
    hung = small.is_alive()
    stop.set()
    big.join(timeout=600)
    assert not hung and not big.is_alive(), "a context did not finish"
    assert not errors, errors
    assert len(small_passes) == 12


@pytest.mark.parametrize("fused", [False, True], ids=["prove_verify", "config5_fused_verify"])
def test_bench_two_ranks_on_one_gpu(fused):
    """`python bench.py --gpus 2` end to end on real hardware: bench.py starts its two ranks itself (torch.distributed.run), both
    ranks share GPU 0 (CPX_BENCH_DEVICE) and meet over gloo (RCCL refuses two ranks on one device), every rank proves and verifies its
    own batch, rank 0 prints ONE line with n_gpus = 2 and the whole-job rate.  With --fused-verify: BASELINE configs[4] across ranks —
    every rank's partial sum of ONE accumulated check, the all-gather of the 148-byte payloads (dist.all_gather_partials) and the
    identity test on every rank.  Small shapes: this checks the plumbing, not the speed."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CPX_BENCH_BACKEND="gloo", CPX_BENCH_DEVICE="0")
    env.setdefault("GLOO_SOCKET_IFNAME", "lo")   # one node: the ranks meet on the loopback interface whatever the box's hostname resolves to
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--ell", "28", "--batch", "128", "--ctxs", "2", "--steps", "2", "--warmup", "1",
           "--full", "--no-extra-shapes", "--no-traffic"] + (["--fused-verify"] if fused else [])
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:   # no second go (round 5 retried once): the whole output of a failed launch is kept for the reader and the test fails
        os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
        with open(os.path.join(root, "gpurun_out", "two_ranks_failure_%s.log" % ("fused" if fused else "prove_verify")), "w") as f:
            f.write("rc=%d\n---- stdout\n%s\n---- stderr\n%s\n" % (r.returncode, r.stdout, r.stderr))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-9000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["all_verified"] is True and d["scaling"] == "weak"
    assert "errors" not in d, d["errors"]   # (a failing extra stage is recorded there instead of taking rank 0 — and the line — down)
    assert d["config"]["global_batch"] == 256 and d["config"]["batch_per_gpu"] == 128
    assert abs(d["value"] - 256 * d["steps"] / (d["ms_per_step"] * 1e-3 * d["steps"])) < 1e-6 * d["value"]
    assert ("batched verifier" in d["metric"]) == fused
    # the N > 1 line is a complete line: the CPU baseline (rank 0 times the oracle while the other ranks wait at the final barrier) and
    # the roofline object sit beside the GPU number in the same run
    assert d["cpu_baseline"] is not None and d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] == 1
    assert d["roofline"] is not None and d["roofline"]["bound"] == "hbm" and d["roofline"]["frac"] > 0 and d["roofline"]["achieved"] > 0
    if not fused:
        assert d["cpu_baseline"]["gpu_proof_bit_exact"] is True
        by_kernel = d["roofline"]["valu"]["isolated_by_kernel"]
        if d["roofline"]["kernel"] in by_kernel:   # one measurement, one number (round 3 printed two)
            assert by_kernel[d["roofline"]["kernel"]]["frac"] == pytest.approx(d["roofline"]["valu"]["isolated"]["frac"], rel=1e-9)


def test_bench_eight_ranks_on_one_gpu():
    """The driver's scaling run ends at N = 8 and is one shot: the same launch with EIGHT real ranks (each with an engine context on GPU 0, gloo instead of
    RCCL, a small shape), not a dry run — eight process-group members, every rank proves and verifies its own batch, the max over ranks, rank 0's
    extras (CPU baseline, roofline) while seven ranks wait at the final barrier, ONE line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CPX_BENCH_BACKEND="gloo", CPX_BENCH_DEVICE="0")
    env.setdefault("GLOO_SOCKET_IFNAME", "lo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--ell", "28", "--batch", "64", "--ctxs", "1", "--steps", "2", "--warmup", "1",
           "--full", "--no-extra-shapes", "--no-traffic"]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-6000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert "errors" not in d, d["errors"]
    assert d["n_gpus"] == 8 and d["all_verified"] is True and d["config"]["global_batch"] == 512 and d["config"]["batch_per_gpu"] == 64
    assert d["cpu_baseline"]["gpu_proof_bit_exact"] is True and d["roofline"]["frac"] > 0


@pytest.mark.parametrize("copies", [1, 97], ids=["host_driven", "device_resident"])
def test_instances_with_identity_points_and_repeated_points(ctx, orc, copies):
    """Edge instances the reference accepts as inputs: a ciphertext whose components are the point at infinity (R_i = S_i = O, hence an
    identity column in the per-proof tables of T and U, an identity base in the R / S MSMs and a 0xc0 encoding in the hashed instance)
    and two identical ciphertexts (equal bases next to each other in every bucket list).  Proof bytes and verdicts must equal the
    oracle's, on the host-driven path (one proof) and on the device-resident path (97 copies of the instance)."""
    import curdleproofs_amd as cpx
    ell = 28
    crs = orc.generate_crs_points(ell)
    base = orc.make_instance(ell, 4242, crs)
    R, S = bytearray(base["vec_R"]), bytearray(base["vec_S"])
    perm = list(base["permutation"])
    i0 = next(i for i in range(ell) if perm.index(i) != 0)            # its image must not land on T[0] (curdleproofs.rs:218 would reject)
    R[i0 * AFF:(i0 + 1) * AFF] = bytes(AFF)
    S[i0 * AFF:(i0 + 1) * AFF] = bytes(AFF)
    a, b = [i for i in range(ell) if i != i0][:2]
    R[b * AFF:(b + 1) * AFF] = R[a * AFF:(a + 1) * AFF]               # two identical ciphertexts
    S[b * AFF:(b + 1) * AFF] = S[a * AFF:(a + 1) * AFF]
    R, S = bytes(R), bytes(S)
    T, U, M = orc.shuffle_permute_and_commit_input(ell, crs, R, S, perm, base["k"], base["vec_m_blinders"])
    want = orc.prove(ell, crs, R, S, T, U, M, perm, base["k"], base["vec_m_blinders"], base["prover_rand"])
    assert orc.verify(ell, crs, R, S, T, U, M, want, base["verifier_rand"]) == 1
    ctx.set_crs(ell, crs)
    ctx.load_batch(R * copies, S * copies, T * copies, U * copies, M * copies)
    proofs = ctx.prove_batch(perm * copies, base["k"] * copies, base["vec_m_blinders"] * copies, base["prover_rand"] * copies)
    assert all(p == want for p in proofs)
    assert ctx.verify_batch(proofs, base["verifier_rand"] * copies) == [cpx.CPX_OK] * copies
    # the same proof against the unmodified instance must fail, as it does for the oracle
    ctx.load_batch(base["vec_R"] * copies, base["vec_S"] * copies, base["vec_T"] * copies, base["vec_U"] * copies, base["M"] * copies)
    assert orc.verify(ell, crs, base["vec_R"], base["vec_S"], base["vec_T"], base["vec_U"], base["M"], want, base["verifier_rand"]) == 0
    assert ctx.verify_batch(proofs, base["verifier_rand"] * copies) == [cpx.CPX_ERR_VERIFY] * copies


def _run_bench(extra, timeout=900, env_extra=None):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **(env_extra or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + extra, env=env, cwd=root, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-6000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert "errors" not in d, d["errors"]
    return d


def test_bench_interleaved_ab_of_an_option_and_of_two_library_builds(tmp_path):
    """bench.py --ab / --ab-lib: the A/B harness alternates blocks of passes between option values on the same contexts, and
    between two builds of the library loaded side by side in one process (here: a byte copy of libcpx.so, so the ratio is a noise figure).  Small
    shapes: this pins the plumbing (every block verified, rates per round, ratios), not a speed."""
    import shutil
    import curdleproofs_amd as cpx
    d = _run_bench(["--ell", "28", "--batch", "128", "--ctxs", "1", "--ab", "fused_rounds_max=0,256", "--ab-rounds", "2", "--ab-passes", "2"])
    ab = d["ab"]
    assert ab["all_verified"] is True and [v["label"] for v in ab["variants"]] == ["fused_rounds_max=0", "fused_rounds_max=256"]
    assert all(len(v["proofs_per_s_by_round"]) == 2 and v["mean"] > 0 for v in ab["variants"]) and ab["variants"][0]["ratio_to_first"] == 1.0
    copy = str(tmp_path / "libcpx_copy.so")
    shutil.copy(cpx._LIB_PATH, copy)
    d = _run_bench(["--ell", "28", "--batch", "256", "--ctxs", "2", "--ab-lib", copy, "--ab-rounds", "2", "--ab-passes", "2"])
    ab = d["ab"]
    assert ab["all_verified"] is True and [v["label"] for v in ab["variants"]] == ["libcpx.so", "libcpx_copy.so"]
    assert 0.5 < ab["variants"][1]["ratio_to_first"] < 2.0


def test_bench_measures_hbm_traffic_in_the_run_and_reports_the_upload_inclusive_rate():
    """The --full bench line's roofline.traffic comes from rocprofv3 --pmc child passes of the run itself (FETCH_SIZE and WRITE_SIZE apart, counters only), the
    whole-pass product fraction and the rate with the public instances uploaded inside the timed region sit beside the headline."""
    d = _run_bench(["--ell", "28", "--batch", "256", "--ctxs", "2", "--steps", "2", "--warmup", "1", "--full", "--no-extra-shapes", "--no-cpu-baseline"])
    r = d["roofline"]
    assert r["traffic"] is not None and r["traffic"] > 0, r["traffic_source"]
    assert r["traffic_source"]["FETCH_SIZE"]["dispatches"] > 0 and r["traffic_source"]["WRITE_SIZE"]["dispatches"] > 0
    assert 0 < r["valu"]["whole_pass"]["frac"] < 1
    assert d["all_verified"] is True and 0.3 < d["instance_upload"]["ratio_to_value"] < 1.5 and d["value_incl_instance_upload"] > 0
    assert d["setup_s"]["total"] > 0


def test_bench_dump_outputs_hold_the_last_steps_proofs(orc, tmp_path):
    """bench.py --dump-outputs DIR: the verdicts and proof bytes the last timed step returned, as float32 .npy.  Two runs of the same command dump the
    same arrays (seeded inputs), and the proof rows are the oracle's proofs of the instances bench.synth_batch draws for rank 0 — across both contexts'
    shares."""
    import sys
    import numpy as np
    import curdleproofs_amd as cpx
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ell, B = 28, 256
    runs = []
    for r in range(2):
        out = tmp_path / ("run%d" % r)
        d = _run_bench(["--ell", str(ell), "--batch", str(B), "--ctxs", "2", "--steps", "2", "--warmup", "1", "--no-extra-shapes", "--no-cpu-baseline",
                        "--no-traffic", "--dump-outputs", str(out)])
        assert d["steps"] == 2 and d["all_verified"] is True and d["ms_per_step"] > 0
        runs.append({f: np.load(out / (f + ".npy")) for f in ("verdicts", "proofs", "proof_index")})
    a, b = runs
    for f in a:
        assert a[f].dtype in (np.float32, np.float64) and np.array_equal(a[f], b[f]), f
    assert a["verdicts"].shape == (B,) and not a["verdicts"].any()
    assert a["proofs"].shape == (B, 48 * (18 + 10 * 5) + 7 * 32) and np.array_equal(a["proof_index"], np.arange(B))
    sys.path.insert(0, root)
    import bench
    c = cpx.Context(0)
    data = bench.synth_batch(c, ell, B, seed=1234)
    for i in (0, 97, B // 2, B - 1):
        it = bench._instance(data, ell, i)
        want = orc.prove(ell, data["crs"], it["vec_R"], it["vec_S"], it["vec_T"], it["vec_U"], it["M"], it["permutation"], it["k"], it["vec_m_blinders"],
                         it["prover_rand"])
        assert bytes(a["proofs"][i].astype(np.uint8)) == want, i
    c.close()


def test_plain_bench_run_prints_the_headline_and_nothing_else():
    """Without --full a run sets up, warms up, times its steps and prints the line: the contract fields, the roofline of the timed region's kernel
    statistics, cpu_baseline null — no extra stage (upload legs, isolated pass, product peak, config 5, shapes, CPU baselines, traffic) runs."""
    d = _run_bench(["--ell", "28", "--batch", "256", "--ctxs", "2", "--steps", "2", "--warmup", "1"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["all_verified"] is True and d["steps"] == 2 and d["warmup"] == 1 and d["dtype"] == "int64" and d["higher_is_better"] is True
    assert abs(d["value"] - 256 * d["steps"] / (d["ms_per_step"] * 1e-3 * d["steps"])) < 1e-6 * d["value"]
    assert d["cpu_baseline"] is None and d["roofline"]["frac"] > 0 and d["roofline"]["traffic"] is None and "valu" not in d["roofline"]
    for k in ("value_incl_instance_upload", "instance_upload", "single_proof", "config5", "baseline_shapes", "ell_508", "ell_1020", "cpu_baseline_all_cores"):
        assert k not in d, k
    s = d["setup_s"]
    assert s["commitments_beside_the_scalar_multiplications"] is True and 0 < s["synthetic_batch"] < s["since_start"]


def test_bench_synthetic_commitments_are_the_points_util_msm_gives():
    """bench.synth_batch commits to every instance at once (bench.commitments: one scale, log2 n folds) on a helper context; every M is the point
    Context.msm gives instance by instance (util.rs:99-103), in Jacobian form with Z = 1."""
    import sys
    import curdleproofs_amd as cpx
    from curdleproofs_amd import params as pr
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    ell, B = 28, 64
    c, h = cpx.Context(0), cpx.Context(0)
    data = bench.synth_batch(c, ell, B, seed=77, helpers=[h])
    idx = [pr.fr_to_wire(i) for i in range(ell)]
    crs_G = data["crs"][:(ell + 4) * AFF]
    for p in range(B):
        sigma = b"".join(idx[i] for i in data["perms"][p * ell:(p + 1) * ell])
        want = c.msm(crs_G, sigma + data["mbl"][p * 4 * FR:(p + 1) * 4 * FR])
        got = data["M"][p * JAC:(p + 1) * JAC]
        assert c.normalize(got) == c.normalize(want), p
        assert got[96:] == pr.fp_to_wire(1), p
    c.close()
    h.close()


def test_staged_instance_upload_keeps_the_loaded_batch_and_then_replaces_it(orc):
    """cpx_batch_load_begin / _end: the NEXT batch's instance is uploaded beside the loaded batch's prove + verify and becomes the loaded batch at
    _end.  Between the two calls the loaded batch still proves to ITS oracle bytes; after _end the staged instances prove to theirs — on the
    host-driven path (3 proofs) and on the device-resident path (64 proofs).  _end without _begin, and a CRS change in between, are state errors."""
    import curdleproofs_amd as cpx
    ell = 28
    crs = orc.generate_crs_points(ell)
    base = [orc.make_instance(ell, 900 + i, crs) for i in range(4)]
    for nb in (3, 64):
        c = cpx.Context(0)
        c.set_crs(ell, crs)
        first = [base[i % 2] for i in range(nb)]            # instances 0 / 1
        second = [base[2 + i % 2] for i in range(nb)]       # instances 2 / 3
        cat = lambda insts, k_: b"".join(i[k_] for i in insts)
        inst = lambda insts: tuple(c.marshal(cat(insts, k_)) for k_ in ("vec_R", "vec_S", "vec_T", "vec_U", "M"))
        wit = lambda insts: ([x for i in insts for x in i["permutation"]], cat(insts, "k"), cat(insts, "vec_m_blinders"), cat(insts, "prover_rand"))
        with pytest.raises(cpx.CpxError) as e:
            c.load_batch_end()
        assert e.value.code == cpx.CPX_ERR_STATE
        c.load_batch(*inst(first))
        staged = inst(second)
        c.load_batch_begin(*staged)
        proofs = c.prove_batch(*wit(first))
        assert [p == i["proof"] for p, i in zip(proofs, first)] == [True] * nb
        assert c.verify_batch(proofs, cat(first, "verifier_rand")) == [cpx.CPX_OK] * nb
        c.load_batch_end()
        assert c.batch == nb
        assert c.verify_batch(proofs, cat(first, "verifier_rand")) == [cpx.CPX_ERR_VERIFY] * nb   # the old proofs do not fit the new instances
        proofs2 = c.prove_batch(*wit(second))
        assert [p == i["proof"] for p, i in zip(proofs2, second)] == [True] * nb
        assert c.verify_batch(proofs2, cat(second, "verifier_rand")) == [cpx.CPX_OK] * nb
        # twice in a row (the staging area is reused once the first staged batch has been copied out), with a smaller batch
        c.load_batch_begin(*inst(first[:2]))
        c.load_batch_end()
        c.load_batch_begin(*inst(second[:2]))
        c.load_batch_end()
        assert c.batch == 2
        assert c.prove_batch(*wit(second[:2])) == [i["proof"] for i in second[:2]]
        # a CRS of another size between _begin and _end: the staged rows no longer fit
        c.load_batch_begin(*inst(first[:2]))
        c.set_crs(60, orc.generate_crs_points(60))
        with pytest.raises(cpx.CpxError) as e:
            c.load_batch_end()
        assert e.value.code == cpx.CPX_ERR_STATE
        c.close()


def test_bench_falls_back_to_fewer_contexts_when_the_default_shape_does_not_fit():
    """bench.py's default is four engine contexts x 8192 proofs (233 of the 288 GB of HBM).  If their set-up or first pass fails (HIP out of memory),
    all ranks together fall back to half the contexts and half the batch and the line says so — rehearsed with the test hook that refuses more than
    two contexts."""
    d = _run_bench(["--ell", "28", "--batch", "256", "--ctxs", "4", "--steps", "2", "--warmup", "1", "--no-extra-shapes", "--no-cpu-baseline", "--no-traffic"],
                   env_extra={"CPX_BENCH_FAIL_SETUP_ABOVE": "2"})
    assert d["config"]["engine_contexts_per_gpu"] == 2 and d["config"]["batch_per_gpu"] == 128 and d["all_verified"] is True
    assert d["config"]["fallback"]["from_contexts"] == 4 and d["config"]["fallback"]["from_batch"] == 256
    assert abs(d["value"] - 128 * d["steps"] / (d["ms_per_step"] * 1e-3 * d["steps"])) < 1e-6 * d["value"]
    d = _run_bench(["--ell", "28", "--batch", "256", "--ctxs", "4", "--steps", "2", "--warmup", "1", "--no-extra-shapes", "--no-cpu-baseline", "--no-traffic"])
    assert d["config"]["engine_contexts_per_gpu"] == 4 and d["config"]["fallback"] is None
