"""The rejecting side of deserialisation on every GPU decoding path, against the reference decoder of tests/decoding_ref.py
(itself pinned to the oracle by tests/test_decoding_reference_cpu.py) and against the oracle's per-proof verdicts.

- cpx_g1_decompress(_status) on both kernels (k_decompress: one lane per point; k_decompress_quad: a quad per point), with and
  without the subgroup test, under both infinity modes, on the bare corpus and on the corpus tiled among valid points past one
  kernel block so that bad points fall on lane 0, lane 63 and the last partial block.
- The DESERIALIZE verdict of every proof and every slot: seven scalar slots with non-canonical and edge-canonical values, every proof
  point slot with a point defect, good proofs on both sides of each bad one; host-driven and device-resident verifier on either
  decompression kernel, and the fused verifier's count of undecodable proofs on the same batches.
- The Whisk entry points with undecodable points and scalars in each role.
Every case reads back the options that select its path."""
import random

import pytest

from tests import decoding_ref as dr

pytestmark = pytest.mark.gpu

AFF = 96
QUAD_DEFAULT = 2048
QUAD_FORCED = 1 << 20


@pytest.fixture(scope="module")
def corpus(orc):
    return dr.corpus(orc)


class _Expect:
    """memoised reference decodes (the subgroup test of the oracle is the slow part)"""

    def __init__(self, orc):
        self.orc, self.memo = orc, {}

    def __call__(self, enc, strict, chk):
        key = (enc, strict, chk)
        if key not in self.memo:
            self.memo[key] = dr.expected_output(enc, self.orc, strict, chk)
        return self.memo[key]


@pytest.fixture(scope="module")
def expect(orc):
    return _Expect(orc)


def _tiled(orc, corpus, n):
    """the corpus three times over among n - 3 * len(corpus) valid subgroup points, shuffled; the encodings refused in every mode
    take lane 0 and lane 63 of several blocks (and the 0 / 15 positions of the quad kernel's blocks), the last partial block
    and the last element"""
    assert n > QUAD_DEFAULT and n % 64
    fill = orc.rng(31337).g1_affine(n)
    encs = [orc.g1_compress(fill[AFF * i:AFF * (i + 1)]) for i in range(n)]
    last_block = n // 64 * 64
    forced = [0, 63, 64, 127, 15, 16, 31, 1024, 1087, 2047, 2048, last_block, last_block + 1, n - 2, n - 1]
    always_bad = [e for _, e in corpus if dr.decode(e, orc, False)[0] and dr.decode(e, orc, False, check_subgroup=False)[0]]
    assert len(always_bad) >= len(forced)
    rnd = random.Random(4711)
    items = [e for _, e in corpus] * 3
    for e in always_bad[:len(forced)]:
        items.remove(e)
    rnd.shuffle(items)
    rest = rnd.sample([i for i in range(n) if i not in forced], len(items))
    for i, e in zip(forced + rest, always_bad[:len(forced)] + items):
        encs[i] = e
    return encs


DECODERS = {"k_decompress": 0, "quad_default": QUAD_DEFAULT, "quad_forced": QUAD_FORCED}


@pytest.mark.parametrize("size", ["corpus", "tiled"])
@pytest.mark.parametrize("decoder", list(DECODERS))
def test_decompress_matches_reference_decoder(orc, corpus, expect, decoder, size):
    import curdleproofs_amd as cpx
    encs = [e for _, e in corpus] if size == "corpus" else _tiled(orc, corpus, 64 * 36 + 37)
    labels = {e: l for l, e in corpus}
    n = len(encs)
    blob = b"".join(encs)
    quad_max = DECODERS[decoder]
    c = cpx.Context(0, options={"decompress_quad_max": quad_max})
    try:
        assert c.get_option("decompress_quad_max") == quad_max
        for strict in (0, 1):
            c.set_option("strict_infinity", strict)
            assert c.get_option("strict_infinity") == strict
            for chk in (False, True):
                kernel = "k_decompress_quad" if (n <= quad_max and chk) else "k_decompress"
                case = "%s n=%d strict_infinity=%d check_subgroup=%d" % (kernel, n, strict, chk)
                want = [expect(e, bool(strict), chk) for e in encs]
                aff, st = c.decompress_status(blob, check_subgroup=chk)
                bad = [(i, labels.get(encs[i], "fill"), st[i], want[i][0]) for i in range(n)
                       if st[i] != want[i][0] or aff[AFF * i:AFF * (i + 1)] != want[i][1]]
                assert not bad, (case, bad[:8])
                if any(w[0] for w in want):
                    with pytest.raises(cpx.CpxError) as e:
                        c.decompress(blob, check_subgroup=chk)
                    assert e.value.code == cpx.CPX_ERR_DESERIALIZE, case
                ok = [i for i in range(n) if want[i][0] == 0]
                assert c.decompress(b"".join(encs[i] for i in ok), check_subgroup=chk) == b"".join(want[i][1] for i in ok), case
                assert st.count(0) == len(ok) < n, case
    finally:
        c.close()


# ---- the proof deserialisation matrix ----

def _put(proof, off, data):
    return proof[:off] + data + proof[off + len(data):]


def _matrix_defects(orc, ell, good, every_point=True):
    """[(label, proof)]: one defect per proof.  every_point: every scalar slot x the six edge values and every point slot with one of
    the five point defects; otherwise every scalar slot with one non-canonical value, every point outside the L-vectors and the first
    and last point of each L-vector"""
    points, scalars = dr.proof_layout(ell)
    L = (ell + 4).bit_length() - 1
    out = []
    nc = list(dr.noncanonical_scalars().items())
    edge = list(nc) + list(dr.canonical_edge_scalars().items())
    for i, slot in enumerate(dr.SCALAR_SLOTS):
        for name, v in (edge if every_point else [nc[i % len(nc)]]):
            out.append(("%s = %s" % (slot, name), _put(good, scalars[slot], v.to_bytes(32, "little"))))
    keep = lambda nm: every_point or "[" not in nm or nm.endswith("[0]") or nm.endswith("[%d]" % (L - 1))
    for q, (nm, off) in enumerate(points):
        if keep(nm):
            kind, enc = dr.point_defects(orc, good[off:off + 48])[q % 5]
            out.append(("%s (slot %d): %s" % (nm, q, kind), _put(good, off, enc)))
    return out


class _Instance:
    def __init__(self, orc, ell, seed, every_point=True):
        self.ell = ell
        self.crs = orc.generate_crs_points(ell)
        self.inst = orc.make_instance(ell, seed, self.crs)
        x = self.inst
        assert x["verdict"] == 1
        self.good = x["proof"]
        self.verdict = lambda pr: orc.verify(ell, self.crs, x["vec_R"], x["vec_S"], x["vec_T"], x["vec_U"], x["M"], pr, x["verifier_rand"])
        self.defects = _matrix_defects(orc, ell, self.good, every_point)
        self.want = [self.verdict(p) for _, p in self.defects]
        for (label, _), w in zip(self.defects, self.want):
            assert w == (0 if ("r-1" in label or "top word" in label) else -1), label


@pytest.fixture(scope="module")
def ell28(orc):
    return _Instance(orc, 28, 21)


def _run_matrix(c, orc, I, B):
    """the defects in batches of B copies of the instance: bad proofs at the odd positions 1, 3, ..., good ones at the first and
    last position and beside every bad one; per-proof verdicts and the fused verifier's undecodable count on each batch"""
    import curdleproofs_amd as cpx
    V = {1: cpx.CPX_OK, 0: cpx.CPX_ERR_VERIFY, -1: cpx.CPX_ERR_DESERIALIZE}   # orc.verify's three answers
    x = I.inst
    c.set_crs(I.ell, I.crs)
    c.load_batch(*(x[k] * B for k in ("vec_R", "vec_S", "vec_T", "vec_U", "M")))
    vrand = x["verifier_rand"] * B
    frand = orc.rng(99).fr(12 * B)
    part, ninv = c.verify_batch_fused_partial([I.good] * B, frand)
    assert ninv == 0 and c.sum_jac(part)[1], "a batch without defects must give the identity partial"
    assert c.verify_batch([I.good] * B, vrand) == [cpx.CPX_OK] * B
    per = (B - 1) // 2
    for s in range(0, len(I.defects), per):
        chunk = list(zip(I.defects[s:s + per], I.want[s:s + per]))
        proofs = [I.good] * B
        want = [cpx.CPX_OK] * B
        label = ["good"] * B
        for j, ((lab, pr), w) in enumerate(chunk):
            proofs[2 * j + 1], want[2 * j + 1], label[2 * j + 1] = pr, V[w], lab
        got = c.verify_batch(proofs, vrand)
        wrong = [(p, label[p], got[p], want[p]) for p in range(B) if got[p] != want[p]]
        assert not wrong, wrong[:8]
        part, ninv = c.verify_batch_fused_partial(proofs, frand)
        assert ninv == sum(1 for _, w in chunk if w == -1), [d[0][0] for d in chunk]
        assert not c.sum_jac(part)[1] or ninv > 0


# (options, B): which decompression kernel and which verifier each batch reaches at ell = 28 (68 proof points per proof)
VERIFY_PATHS = {
    "host_driven_quad": ({}, 29),                                                            # 29 * 68 = 1972 <= 2048, 29 < 56
    "host_driven_k_decompress": ({}, 40),                                                    # 2720 > 2048
    "device_resident_k_decompress": ({}, 97),                                                # 97 >= 56
    "device_resident_quad": ({"device_min_batch": 1, "decompress_quad_max": QUAD_FORCED}, 29),
}


@pytest.mark.parametrize("path", list(VERIFY_PATHS))
def test_proof_deserialisation_verdict_per_proof_and_slot(orc, ell28, path):
    import curdleproofs_amd as cpx
    opts, B = VERIFY_PATHS[path]
    c = cpx.Context(0, options=opts)
    try:
        npts = B * len(dr.proof_layout(28)[0])
        dmb, qmax = c.get_option("device_min_batch"), c.get_option("decompress_quad_max")
        assert c.get_option("strict_infinity") == 0
        assert (B >= dmb) == path.startswith("device_resident")
        assert (npts <= qmax) == path.endswith("_quad")
        _run_matrix(c, orc, ell28, B)
    finally:
        c.close()


def test_proof_deserialisation_ell252_host_driven_k_decompress(orc):
    import curdleproofs_amd as cpx
    I = _Instance(orc, 252, 3, every_point=False)
    points = dict(dr.proof_layout(252)[0])
    labels = [l for l, _ in I.defects]
    assert all(any(l.startswith(s + " = ") for l in labels) for s in dr.SCALAR_SLOTS)
    assert all(any(l.startswith("%s[%d] " % (v, j)) for l in labels) for v in dr.L_VECTORS for j in (0, 7)) and len(points) == 98
    B = 40
    c = cpx.Context(0)
    try:
        assert B < c.get_option("device_min_batch") and B * 98 > c.get_option("decompress_quad_max")
        _run_matrix(c, orc, I, B)
    finally:
        c.close()


# ---- Whisk ----

def _tracker_case(orc):
    gen = orc.g1_generator()
    rng = orc.rng(0)
    k, r = rng.fr(1), rng.fr(1)
    rG = orc.g1_scale(gen, r)
    tracker = orc.g1_compress(rG) + orc.g1_compress(orc.g1_scale(rG, k))
    k_commitment = orc.g1_compress(orc.g1_scale(gen, k))
    proof = orc.generate_whisk_tracker_proof(tracker, k, rng.fr(1))
    return tracker, k_commitment, proof


def _bad_points(orc):
    nm = dr.non_member_points(orc, 1)[0]
    return [("outside the subgroup", dr.encode(nm[0], 0x80)), ("x = p", dr.encode(dr.P, 0x80))]


def test_whisk_tracker_proof_refuses_undecodable_inputs(orc):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    tracker, kc, proof = _tracker_case(orc)
    c = cpx.Context(0)
    try:
        T = lambda t: whisk.WhiskTracker(t[:48], t[48:])
        assert orc.is_valid_whisk_tracker_proof(tracker, kc, proof) == 1 and whisk.is_valid_whisk_tracker_proof(c, T(tracker), kc, proof)
        cases = []
        for kind, enc in _bad_points(orc):
            cases += [("r_G " + kind, _put(tracker, 0, enc), kc, proof), ("k_r_G " + kind, _put(tracker, 48, enc), kc, proof),
                      ("k_commitment " + kind, tracker, enc, proof),
                      ("A " + kind, tracker, kc, _put(proof, 0, enc)), ("B " + kind, tracker, kc, _put(proof, 48, enc))]
        cases.append(("s = r", tracker, kc, _put(proof, 96, dr.R.to_bytes(32, "little"))))
        for label, t, k, p in cases:
            assert orc.is_valid_whisk_tracker_proof(t, k, p) == -1, label
            with pytest.raises(whisk.SerializationError):
                whisk.is_valid_whisk_tracker_proof(c, T(t), k, p)
    finally:
        c.close()


@pytest.fixture(scope="module")
def whisk_shuffle_case(orc, whisk_kat):
    ell = 124
    v, proof, pre, post = orc.kat_shuffle_proof(ell)
    assert v == 1 and proof == bytes.fromhex(whisk_kat["whisk_shuffle_proof_ell124"])
    return ell, orc.generate_crs_points(ell), pre, post, proof


@pytest.mark.parametrize("quad_max", [QUAD_DEFAULT, 0], ids=["quad_kernel", "k_decompress"])
def test_whisk_shuffle_proof_refuses_undecodable_inputs(orc, whisk_shuffle_case, quad_max):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    ell, crs, pre, post, proof = whisk_shuffle_case
    rand = orc.rng(123).fr(8)
    trackers = lambda b: [whisk.WhiskTracker(b[96 * i:96 * i + 48], b[96 * i + 48:96 * i + 96]) for i in range(ell)]
    c = cpx.Context(0, options={"decompress_quad_max": quad_max})
    try:
        assert c.get_option("decompress_quad_max") == quad_max
        c.set_crs(ell, crs)
        assert whisk.is_valid_whisk_shuffle_proof(c, trackers(pre), trackers(post), proof, rand=rand)
        cases = []
        for kind, enc in _bad_points(orc):
            cases += [("pre[0].r_G " + kind, _put(pre, 0, enc), post, proof),
                      ("pre[61].k_r_G " + kind, _put(pre, 96 * 61 + 48, enc), post, proof),
                      ("post[123].r_G " + kind, pre, _put(post, 96 * 123, enc), proof),
                      ("post[31].k_r_G " + kind, pre, _put(post, 96 * 31 + 48, enc), proof),
                      ("M " + kind, pre, post, _put(proof, 0, enc))]
        cases.append(("post[7].r_G x = 0", pre, _put(post, 96 * 7, dr.encode(0, 0x80)), proof))
        for label, a, b, p in cases:
            assert orc.is_valid_whisk_shuffle_proof(ell, crs, a, b, p, rand) == -1, label
            with pytest.raises(whisk.SerializationError):
                whisk.is_valid_whisk_shuffle_proof(c, trackers(a), trackers(b), p, rand=rand)
        assert whisk.is_valid_whisk_shuffle_proof(c, trackers(pre), trackers(post), proof, rand=rand)
    finally:
        c.close()
