"""Pins the reference decoder of tests/decoding_ref.py to the oracle (orc.g1_decompress, both infinity modes) on the whole
corpus, before tests/test_gpu_decoding.py uses it to judge the GPU decoders.  CPU only."""
import pytest

from tests import decoding_ref as dr


@pytest.fixture(scope="module")
def corpus(orc):
    return dr.corpus(orc)


def test_corpus_covers_every_edge(orc, corpus):
    encs = [e for _, e in corpus]
    assert len(set(encs)) == len(encs), "duplicate encodings"
    for strict in (False, True):
        st = [dr.decode(e, orc, strict)[0] for e in encs]
        assert st.count(dr.OK) >= 12 and st.count(dr.MALFORMED) >= 40 and st.count(dr.NOT_IN_SUBGROUP) >= 10
    assert {e[0] for e in encs} >= set(dr.FLAG_BYTES)
    labels = dict(corpus)
    # (0, +-2) is on the curve and 3-torsion: outside the subgroup under either sort bit
    assert dr.decode(labels["x=0 flags 80"], orc) == (dr.NOT_IN_SUBGROUP, None, None)
    assert dr.decode(labels["x=0 flags a0"], orc) == (dr.NOT_IN_SUBGROUP, None, None)
    assert dr.decode(labels["x=0 flags 80"], orc, check_subgroup=False) == (dr.OK, 0, 2)
    assert dr.decode(labels["x=0 flags a0"], orc, check_subgroup=False) == (dr.OK, 0, dr.P - 2)
    assert not dr.is_qr(3)   # x = p - 1: x^3 + 4 = 3 is a non-residue
    for name in ("x=p-1", "x=p", "x=p+1", "x=2^381-1"):
        for f in (0x80, 0xa0):
            assert dr.decode(labels["%s flags %02x" % (name, f)], orc)[0] == dr.MALFORMED, name


def test_no_two_torsion():
    # y = 0 needs x^3 = -4; -4 is not a cube in Fp (p = 1 mod 3), so the sort flag always has two distinct roots to pick from
    assert dr.P % 3 == 1 and pow(dr.P - 4, (dr.P - 1) // 3, dr.P) != 1


def test_sort_flag_picks_the_larger_root_and_flipping_it_negates(orc):
    for i, pt in enumerate(dr.subgroup_points(orc, 6)):
        enc = dr.compress(pt)
        assert enc == orc.g1_compress(dr.aff_wire(pt))
        st, x, y = dr.decode(enc, orc)
        assert st == dr.OK and (x, y) == pt
        st, x2, y2 = dr.decode(bytes([enc[0] ^ 0x20]) + enc[1:], orc)
        assert st == dr.OK and (x2, y2) == (pt[0], dr.P - pt[1])
        assert (y > dr.P - y) == bool(enc[0] & 0x20)


@pytest.mark.parametrize("strict", [False, True], ids=["ark_0_4_infinity", "strict_infinity"])
def test_reference_decoder_matches_oracle_on_the_corpus(orc, corpus, strict):
    orc.set_strict_infinity(strict)
    try:
        for label, enc in corpus:
            st, x, y = dr.decode(enc, orc, strict)
            try:
                got = orc.g1_decompress(enc)
            except ValueError:
                got = None
            if st == dr.OK:
                assert got == dr.aff_wire(None if x is None else (x, y)), label
            else:
                assert got is None, label
            # without the subgroup test the same decoder accepts exactly the on-curve points outside the subgroup too
            st0, x0, y0 = dr.decode(enc, orc, strict, check_subgroup=False)
            assert st0 == (dr.OK if st == dr.NOT_IN_SUBGROUP else st), label
            if st == dr.NOT_IN_SUBGROUP:
                w = dr.aff_wire((x0, y0))
                assert orc.g1_on_curve(w) and not orc.g1_in_subgroup(w), label
    finally:
        orc.set_strict_infinity(False)


def test_expected_output_writes_the_identity_for_rejected_points(orc, corpus):
    for label, enc in corpus:
        for strict in (False, True):
            for chk in (False, True):
                st, aff = dr.expected_output(enc, orc, strict, chk)
                if st:
                    assert aff == bytes(dr.AFF), label


def test_proof_layout_matches_the_parity_tests_offsets():
    from tests.test_gpu_parity import _proof_offsets
    for ell in (28, 124, 252):
        points, scalars = dr.proof_layout(ell)
        off = _proof_offsets(ell)
        assert scalars == {k: off[k] for k in dr.SCALAR_SLOTS}
        at = dict(points)
        L = (ell + 4).bit_length() - 1
        for v in dr.L_VECTORS:
            assert at["%s[0]" % v] == off[v] and at["%s[%d]" % (v, L - 1)] == off[v] + 48 * (L - 1)
        for a, b in (("A", "A"), ("cm_T.T1", "cm_T_T1"), ("cm_U.T2", "cm_U_T2"), ("B", "B"), ("C", "C"), ("B_c", "B_c"), ("B_d", "B_d"),
                     ("cm_A.T1", "cm_A_T1"), ("cm_B.T2", "cm_B_T2"), ("B_a", "B_a"), ("B_u", "B_u")):
            assert at[a] == off[b]


def test_point_defects_are_refused_by_the_oracle(orc):
    original = orc.g1_compress(orc.g1_generator())
    for name, enc in dr.point_defects(orc, original):
        assert dr.decode(enc, orc)[0] != dr.OK, name
        with pytest.raises(ValueError):
            orc.g1_decompress(enc)
    for name, v in dr.noncanonical_scalars().items():
        assert v >= dr.R
        with pytest.raises(ValueError):
            orc.fr_from_canonical_bytes(v.to_bytes(32, "little"))
    for name, v in dr.canonical_edge_scalars().items():
        assert v < dr.R and (v >> 224) == (dr.R >> 224) - 1 or v == dr.R - 1
        orc.fr_from_canonical_bytes(v.to_bytes(32, "little"))
