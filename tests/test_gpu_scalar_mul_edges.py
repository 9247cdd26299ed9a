"""The edge scalars of tests/scalar_cases.py through the kernels built on the recodings: ctx.scale and ctx.fold (k_smul<false>, the
endomorphism-split form and the 257-step plain form of option scale_any_point) and the batched shuffle step at ell = 28 (k_smul_quad up
to smul_quad_max elements, the one-lane k_smul beyond or with smul_quad_max = 0).  Expected bytes come from the oracle alone
(g1_scale, g1_fold, shuffle_permute_and_commit_input).  The scalars turn the signs of k and of t ((r +- 1) / 2, z^2 / 2), empty one half
of the split (t = 0, q = 0), reach the longest digit streams, and select each of the eight table entries of k_smul_quad at the top step."""
import pytest

from tests import scalar_cases as sc
from tests.scalar_cases import R, Z2, H2

pytestmark = pytest.mark.gpu

AFF, FR, ELL = 96, 32, 28
N = 64 + 5                         # one full wave and a wave with 59 dead lanes

# the eight table entries of k_smul_quad at the top step (tracker_ladder.hpp order): k' = q z^2 +- t with the longer half on top, or both
# halves of one length; k = k' or r - k'
_B = 1 << 100
TOP_ENTRY_SCALARS = [3 * Z2 + _B, R - (3 * Z2 + _B), _B * Z2 + 3, R - (_B * Z2 + 3), _B * Z2 + _B, R - (_B * Z2 + _B), R - (_B * Z2 - _B), _B * Z2 - _B]


def top_entry(k):
    """the table entry (d P + d' N P, tracker_ladder.hpp numbering) of the highest step at which k has a digit, from the Python split"""
    t, q, nk, nt = sc.py_split(k)
    dt, dq = sc.naf(t), sc.naf(q)
    top = max(len(dt), len(dq)) - 1
    a = (dt[top] if top < len(dt) else 0) * (-1 if nk ^ nt else 1)
    b = (dq[top] if top < len(dq) else 0) * (-1 if nk else 1)
    return {(1, 0): 0, (-1, 0): 1, (0, 1): 2, (0, -1): 3, (1, 1): 4, (-1, -1): 5, (1, -1): 6, (-1, 1): 7}[(a, b)]


def edge_scalars():
    return list(sc.EDGE_SCALARS.values()) + TOP_ENTRY_SCALARS


def pattern_scalars():
    """the byte and nibble patterns (0x80, 0x7f, 0x88, 0x99, 0x55, 0xaa, 0x33, ...: the longest carry runs of the non-adjacent form) and, for
    every fixed-base width, the scalars with all windows at / around the carry threshold: N of them"""
    out = sc.pattern_scalars() + [v for cb in sc.FIX_CB for v in sc.threshold_scalars(cb)[-3:]]
    out += [(1 << b) - 1 for b in (127, 128, 129, 253, 254)] + [1 << b for b in (126, 128, 129, 253)]
    out += sc.threshold_scalars(19)                   # single windows at the threshold under a run of ones, to fill the second wave
    return out[:N]


def _fr(orc, v):
    return orc.fr_from_canonical_bytes((v % R).to_bytes(32, "little"))


def test_top_entry_scalars_select_all_eight_entries():
    assert [top_entry(k) for k in TOP_ENTRY_SCALARS] == list(range(8))
    assert all(0 < k < R for k in TOP_ENTRY_SCALARS)


@pytest.fixture(scope="module")
def points(orc):
    rng = orc.rng(7301)
    pts = bytearray(rng.g1_affine(N))
    pts[5 * AFF:6 * AFF] = bytes(AFF)                 # one identity point
    return bytes(pts)


@pytest.fixture(scope="module", params=[0, 1], ids=["split", "plain"])
def sctx(request):
    import curdleproofs_amd as cpx
    c = cpx.Context(0)
    c.set_option("scale_any_point", request.param)
    yield c
    c.close()


def test_scale_edge_scalars_per_element(sctx, orc, points):
    ks = edge_scalars()
    assert len(ks) <= N
    rounds = [[ks[(i + s) % len(ks)] for i in range(N)] for s in (0, 7)]      # every edge scalar on two points, one lands on the identity
    assert any(r[5] for r in rounds)
    pats = pattern_scalars()
    assert len(pats) == N and all(0 <= k < R for k in pats) and all(int(b * 32, 16) % R in pats for b in ("55", "aa", "33", "80", "7f", "88", "99"))
    for r in rounds + [pats]:
        scalars = b"".join(_fr(orc, k) for k in r)
        got, want = sctx.scale(points, scalars), orc.g1_scale(points, scalars)
        for i in range(N):
            assert got[AFF * i:AFF * (i + 1)] == want[AFF * i:AFF * (i + 1)], "element %d, k = %s" % (i, hex(r[i]))
    assert got[5 * AFF:6 * AFF] == bytes(AFF)


def test_scale_edge_scalar_shared(sctx, orc, points):
    for name, k in list(sc.EDGE_SCALARS.items()) + [("top entry %d" % e, k) for e, k in enumerate(TOP_ENTRY_SCALARS)]:
        s = _fr(orc, k)
        assert sctx.scale(points, s) == orc.g1_scale(points, s), name


GAMMAS = {"0": 0, "1": 1, "r-1": R - 1, "z2/2": H2, "z2/2+1": H2 + 1, "z2": Z2, "(r-1)/2": (R - 1) // 2, "(r+1)/2": (R + 1) // 2}


@pytest.mark.parametrize("name", list(GAMMAS))
def test_fold_edge_gammas_with_doubling_and_cancelling_elements(sctx, orc, name):
    """PL + gamma PR where the closing mixed addition doubles (PL = gamma PR, in the first and in the second wave), cancels
    (PL = -gamma PR), and where PL, PR or both are the identity, all in one call"""
    g = GAMMAS[name]
    rng = orc.rng(7400 + len(name))
    PL, PR = bytearray(rng.g1_affine(N)), bytearray(rng.g1_affine(N))
    gamma, minus = _fr(orc, g), _fr(orc, R - g)
    el = lambda b, i: bytes(b[AFF * i:AFF * (i + 1)])
    for i in (0, 63, 64, N - 1):
        PL[AFF * i:AFF * (i + 1)] = orc.g1_scale(el(PR, i), gamma)            # a doubling
    for i in (1, 65):
        PL[AFF * i:AFF * (i + 1)] = orc.g1_scale(el(PR, i), minus)            # identity out
    PL[2 * AFF:3 * AFF] = bytes(AFF)
    PR[3 * AFF:4 * AFF] = bytes(AFF)
    PL[4 * AFF:5 * AFF] = PR[4 * AFF:5 * AFF] = bytes(AFF)
    got, want = sctx.fold(bytes(PL), bytes(PR), gamma), orc.g1_fold(bytes(PL), bytes(PR), gamma)
    for i in range(N):
        assert got[AFF * i:AFF * (i + 1)] == want[AFF * i:AFF * (i + 1)], "element %d" % i
    assert el(got, 1) == el(got, 65) == el(got, 4) == bytes(AFF)
    if g:
        assert el(got, 0) != bytes(AFF) and el(got, 0) == orc.g1_scale(el(PR, 0), _fr(orc, 2 * g))


# ---- k_smul_quad through the batched shuffle step ----
@pytest.fixture(scope="module")
def shuffles(orc):
    """one shuffle per edge scalar as the caller's k, with the oracle's result.  util.rs:83-106 rejects no k (k = 0 gives identities),
    so none is left out."""
    crs = orc.generate_crs_points(ELL)
    rng = orc.rng(7500)
    items = []
    for k in edge_scalars():
        vec_R = rng.g1_affine(ELL)
        it = dict(k=k, kb=_fr(orc, k), vec_R=vec_R, vec_S=orc.g1_scale(vec_R, rng.fr(ELL)), perm=rng.shuffle(ELL), mb=rng.fr(4))
        it["want"] = orc.shuffle_permute_and_commit_input(ELL, crs, it["vec_R"], it["vec_S"], it["perm"], it["kb"], it["mb"])
        items.append(it)
    return crs, items


@pytest.mark.parametrize("quad_max", [1024, 0], ids=["quad", "one_lane"])
def test_shuffle_step_with_edge_k(orc, shuffles, quad_max):
    """Calls of 17 and at most 17 items: 2 x 17 x 28 = 952 elements stay at or below the default smul_quad_max = 1024 (18 items, 1008
    elements, are the most), so launch_smul takes k_smul_quad, 59.5 waves of 16 quads: the last wave has dead quads.  The same calls on a
    context with smul_quad_max = 0 take the one-lane k_smul.  The profile times either form as "k_smul" and counts a launch that
    launch_smul ran as k_smul_quad under "k_smul_quad" as well: one of each per call on the first context, none of the latter on the second."""
    import curdleproofs_amd as cpx
    from curdleproofs_amd import util
    crs, items = shuffles
    c = cpx.Context(0, options={} if quad_max else {"smul_quad_max": 0})
    try:
        c.set_crs(ELL, crs)
        assert c.get_option("smul_quad_max") == quad_max and c.get_option("scale_any_point") == 0
        c.set_profiling(True)
        for lo in range(0, len(items), 17):
            it = items[lo:lo + 17]
            elements = 2 * len(it) * ELL
            assert elements <= 1024 and (len(it) < 17 or elements % 16)
            c.reset_stats()
            got = util.shuffle_permute_and_commit_inputs(c, [x["vec_R"] for x in it], [x["vec_S"] for x in it], [x["perm"] for x in it], [x["kb"] for x in it],
                                                         [x["mb"] for x in it])
            assert (c.stat("k_smul")["launches"], c.stat("k_smul_quad")["launches"]) == (1, 1 if quad_max else 0)
            for x, (t, u, m) in zip(it, got):
                assert t == x["want"][0] and u == x["want"][1], "k = %s" % hex(x["k"])
                assert orc.g1_compress_jac(m) == orc.g1_compress_jac(x["want"][2]), "M, k = %s" % hex(x["k"])
    finally:
        c.close()
    assert {top_entry(x["k"]) for x in items if x["k"]} == set(range(8))
