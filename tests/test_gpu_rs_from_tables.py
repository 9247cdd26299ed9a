"""The device-resident prover's R and S from the per-proof tables (option rs_from_tables, engine_device.cpp; prove_reqs.hpp
prove_rs_tables): k R = msm(vec_T, a_sigma), k S = msm(vec_U, a_sigma), then R = k^-1 (k R), cm_T.T_2 = k R + r_t H, cm_A.T_2 =
(r_k k^-1) (k R) + r_a H and the same for S — against the oracle's bytes, on both layouts of the per-proof tables (one segment up to
fused_smsm_max proofs, two above), beside the one-off bucket MSMs (option 0), with the batches that fall back (a k = 0) and with a
witness for which the two ways differ (vec_T != k sigma(vec_R))."""
import pytest

from tests.oracle_lib import AFF, FR

pytestmark = pytest.mark.gpu

ELL = 28
R_MODULUS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001   # the order of G1 (BLS12-381)


def _reproved(orc, crs, base, vec_R=None, permutation=None, k=None):
    """the instance `base` with another vec_R / permutation / k: T, U, M as shuffle_permute_and_commit_input makes them, the oracle's proof"""
    x = dict(base)
    x["vec_R"] = base["vec_R"] if vec_R is None else vec_R
    x["permutation"] = base["permutation"] if permutation is None else permutation
    x["k"] = base["k"] if k is None else k
    x["vec_T"], x["vec_U"], x["M"] = orc.shuffle_permute_and_commit_input(ELL, crs, x["vec_R"], x["vec_S"], x["permutation"], x["k"], x["vec_m_blinders"])
    return _oracle_proof(orc, crs, x)


def _oracle_proof(orc, crs, x):
    x["proof"] = orc.prove(ELL, crs, x["vec_R"], x["vec_S"], x["vec_T"], x["vec_U"], x["M"], x["permutation"], x["k"], x["vec_m_blinders"], x["prover_rand"])
    x["verdict"] = orc.verify(ELL, crs, x["vec_R"], x["vec_S"], x["vec_T"], x["vec_U"], x["M"], x["proof"], x["verifier_rand"])
    return x


@pytest.fixture(scope="module")
def world(orc):
    """the oracle's side, computed once: distinct consistent instances (among them one with the identity permutation and one whose vec_R
    has an identity entry), one with k = 0 and one whose k was replaced by k + 1 after T and U were made"""
    crs = orc.generate_crs_points(ELL)
    plain = [orc.make_instance(ELL, 4100 + s, crs) for s in range(8)]
    ident_perm = _reproved(orc, crs, plain[0], permutation=list(range(ELL)))
    # an identity entry of vec_R that the permutation does not bring to position 0 (the verifier refuses vec_T[0] = O, curdleproofs.rs:218)
    at = plain[1]["permutation"][1]
    R = plain[1]["vec_R"]
    ident_entry = _reproved(orc, crs, plain[1], vec_R=R[:at * AFF] + bytes(AFF) + R[(at + 1) * AFF:])
    assert ident_entry["vec_T"][AFF:2 * AFF] == bytes(AFF) and ident_entry["vec_T"][:AFF] != bytes(AFF)
    good = plain[2:] + [ident_perm, ident_entry]
    assert all(x["verdict"] == 1 for x in good)
    zero_k = _reproved(orc, crs, plain[0], k=bytes(FR))
    assert zero_k["vec_T"] == bytes(ELL * AFF)
    k1 = (int.from_bytes(orc.fr_to_canonical_bytes(plain[1]["k"]), "little") + 1) % R_MODULUS
    wrong_k = dict(plain[1])
    wrong_k["k"] = orc.fr_from_canonical_bytes(k1.to_bytes(32, "little"))
    wrong_k = _oracle_proof(orc, crs, wrong_k)
    assert wrong_k["verdict"] == 0 and wrong_k["proof"] != plain[1]["proof"]
    return dict(crs=crs, good=good, zero_k=zero_k, wrong_k=wrong_k)


@pytest.fixture(scope="module")
def ctxs(world):
    """a context per way: 1 = from the tables (the default), 0 = the one-off bucket MSMs, "two" = those as two tasks per proof"""
    import curdleproofs_amd as cpx
    assert cpx.Context(0).get_option("rs_from_tables") == 1, "the default"
    made = {1: cpx.Context(0, options={"rs_from_tables": 1}), 0: cpx.Context(0, options={"rs_from_tables": 0}),
            "two": cpx.Context(0, options={"rs_from_tables": 0, "rs_pairs": 0})}
    for c in made.values():
        c.set_crs(ELL, world["crs"])
        c.set_profiling(True)
    yield made
    for c in made.values():
        c.close()


def _prove(c, insts):
    cat = lambda key: b"".join(x[key] for x in insts)
    c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
    c.reset_stats()
    proofs = c.prove_batch([i for x in insts for i in x["permutation"]], cat("k"), cat("vec_m_blinders"), cat("prover_rand"))
    # (read before the verifier runs: its accumulated check is a bucket MSM of the same kernel family)
    c.prover_bucket_msms = c.stat("k_msm_tblw_pair")["launches"] + c.stat("k_msm_tblw<2, true>")["launches"]
    assert c.stat("k_smul")["launches"] == 1
    return proofs, c.verify_batch(proofs, cat("verifier_rand"))


def _sizes(c):
    """a batch on each side of fused_smsm_max (kernels.h): one-segment tables up to it, two-segment tables above"""
    fm = c.get_option("fused_smsm_max")
    assert c.get_option("device_min_batch") <= fm < c.get_option("late_min_batch") - 1 and c.get_option("tbl_segments") == 0
    return {"one_segment": (fm, 1), "two_segments": (fm + 1, 2)}


def _batch(pool, count, at=0):
    return [pool[(at + i) % len(pool)] for i in range(count)]


def _ran(c, from_tables):
    assert c.prover_bucket_msms == (0 if from_tables else 1), "the one-off bucket MSMs run exactly when R and S do not come from the tables"


@pytest.mark.parametrize("layout", ["one_segment", "two_segments"])
@pytest.mark.parametrize("way", [1, 0, "two"])
def test_consistent_witnesses_give_the_oracles_bytes(ctxs, world, way, layout):
    import curdleproofs_amd as cpx
    c = ctxs[way]
    count, segments = _sizes(c)[layout]
    insts = _batch(world["good"], count)
    proofs, verdicts = _prove(c, insts)
    assert c.get_option("tbl_segments_effective") == segments
    _ran(c, way == 1)
    wrong = [i for i, (x, p) in enumerate(zip(insts, proofs)) if p != x["proof"]]
    assert not wrong, "proofs %s... differ from the oracle's" % wrong[:8]
    assert verdicts == [cpx.CPX_OK] * count


@pytest.mark.parametrize("layout", ["one_segment", "two_segments"])
def test_a_batch_with_a_zero_k_takes_the_bucket_msms(ctxs, world, layout):
    """k = 0 has no inverse: the whole batch falls back, and every proof — that of the k = 0 witness (T and U all identity, which the
    reference proves) included — equals the oracle's"""
    import curdleproofs_amd as cpx
    c = ctxs[1]
    count, _ = _sizes(c)[layout]
    insts = _batch(world["good"], count, at=3)
    insts[count // 2] = world["zero_k"]
    proofs, verdicts = _prove(c, insts)
    _ran(c, False)
    assert [p == x["proof"] for x, p in zip(insts, proofs)] == [True] * count
    assert [v == cpx.CPX_OK for v in verdicts] == [x["verdict"] == 1 for x in insts]
    # the next batch without one is back on the tables
    _prove(c, _batch(world["good"], count))
    _ran(c, True)


@pytest.mark.parametrize("layout", ["one_segment", "two_segments"])
def test_an_inconsistent_witness(ctxs, world, layout):
    """vec_T != k sigma(vec_R) (k replaced by k + 1): no proof for it verifies.  The bucket MSMs emit the reference's bytes; from the tables
    R, S and the T_2 commitments are other points, hence another proof, which the verifier refuses as well.  The other proofs of the
    batch are the oracle's either way."""
    import curdleproofs_amd as cpx
    at = 5
    for way in (0, 1):
        c = ctxs[way]
        count, _ = _sizes(c)[layout]
        insts = _batch(world["good"], count, at=1)
        insts[at] = world["wrong_k"]
        proofs, verdicts = _prove(c, insts)
        _ran(c, way == 1)
        same = [p == x["proof"] for x, p in zip(insts, proofs)]
        assert same == [i != at or way == 0 for i in range(count)]
        assert verdicts == [cpx.CPX_ERR_VERIFY if i == at else cpx.CPX_OK for i in range(count)]
