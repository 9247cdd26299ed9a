"""GPU parity of the per-round tier-0 calls: Context.msm_many -> cpx_g1_msm_many (the cross terms of a log round in one call) and
Context.fold_many -> cpx_g1_fold_many (its basis folds in one call).  Expected values come from the oracle — g1_msm, g1_fold, g1_scale,
g1_compress_jac, g1_eq_jac — never from the library under test; the single calls (ctx.msm) are only compared WITH.  The length lists put
empty tasks, one point, the 64-point slab boundary, several slabs and ragged neighbours behind one launch; (1030, 5, 0, 64) is the
smallest call for which the slice rule picks 4 waves per window (tests/test_tier0_rounds_cpu.py restates the rule)."""
import ctypes
import random

import pytest

pytestmark = pytest.mark.gpu

FR, AFF, JAC = 32, 96, 144
R_ = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
IDENTITY = bytes([0xc0]) + bytes(47)
RAGGED = (0, 1, 2, 15, 16, 17, 63, 64, 65, 129)
LISTS = {"ragged": RAGGED, "ragged_reversed": RAGGED[::-1], "smsm_round_6x64": (64,) * 6, "ipa_round_ell252": (129, 128, 129, 128), "one_task": (7,),
         "forty_of_3": (3,) * 40}
SLICED = (1030, 5, 0, 64)
FOLD_FAMILIES, FOLD_HALVES = (1, 2, 3), (1, 2, 5, 16, 17, 64, 128)
FORMS = {"default": ({}, 1), "fold_quad_max_0": ({"fold_quad_max": 0}, 0), "scale_any_point": ({"scale_any_point": 1}, 0)}      # options, k_smul_quad launches per call
POOL = 1100


def _wire(orc, ints):
    return orc.fr_from_canonical_bytes(b"".join((v % R_).to_bytes(32, "little") for v in ints))


def _pt(buf, i, n=1):
    return buf[AFF * i:AFF * (i + n)]


def _sc(buf, i, n=1):
    return buf[FR * i:FR * (i + n)]


@pytest.fixture(scope="module")
def ctx():
    import curdleproofs_amd as cpx
    c = cpx.Context(0)
    yield c
    c.close()


class Pool:
    """seeded oracle points and scalars; tasks of a length list are consecutive ranges of them, so neighbours differ"""

    def __init__(self, orc):
        rng = orc.rng(20261019)
        self.points = rng.g1_affine(POOL)
        self.scalars = rng.fr(POOL)
        self.orc = orc
        self._msm = {}

    def tasks(self, lens):
        out, off = [], 0
        for n in lens:
            if off + n > POOL:
                off = 0
            out.append((_pt(self.points, off, n), _sc(self.scalars, off, n)))
            off += n
        return out

    def msm(self, bases, scalars):
        key = (bases, scalars)
        if key not in self._msm:
            self._msm[key] = self.orc.g1_msm(bases, scalars)
        return self._msm[key]


@pytest.fixture(scope="module")
def pool(orc):
    return Pool(orc)


def _check_msm_many(ctx, orc, pool, tasks, against_single=True):
    jac, comp = ctx.msm_many([b for b, _ in tasks], [s for _, s in tasks], compressed=True)
    assert len(jac) == len(comp) == len(tasks)
    for i, (b, s) in enumerate(tasks):
        want = pool.msm(b, s)
        assert len(jac[i]) == JAC and comp[i] == orc.g1_compress_jac(want), "task %d of %d points" % (i, len(s) // FR)
        assert orc.g1_eq_jac(jac[i], want), "task %d of %d points" % (i, len(s) // FR)
        if against_single:
            assert orc.g1_eq_jac(jac[i], ctx.msm(b, s)), "task %d: cpx_g1_msm on the task alone" % i
        if not s:
            assert jac[i][96:] == bytes(48) and comp[i] == IDENTITY          # an empty task: Z == 0, 0xc0 || 0^47
    assert ctx.msm_many([b for b, _ in tasks], [s for _, s in tasks]) == jac
    return jac, comp


# ---- MSM ----
@pytest.mark.parametrize("name", list(LISTS))
def test_msm_many_ragged_lengths_match_the_oracle_and_the_single_call(ctx, orc, pool, name):
    _check_msm_many(ctx, orc, pool, pool.tasks(LISTS[name]))


def test_msm_many_either_output_may_be_null(ctx, orc, pool):
    import curdleproofs_amd as cpx
    L, h = ctx._L, ctx._h
    tasks = pool.tasks((5, 0, 64))
    n = len(tasks)
    lens = (ctypes.c_uint32 * n)(*(len(s) // FR for _, s in tasks))
    bases, scalars = cpx._in(b"".join(b for b, _ in tasks)), cpx._in(b"".join(s for _, s in tasks))
    want = [pool.msm(b, s) for b, s in tasks]
    fill = lambda size: (ctypes.c_uint8 * size)(*([0xaa] * size))
    j, c = fill(JAC * n), fill(48 * n)
    assert L.cpx_g1_msm_many(h, n, lens, bases, scalars, j, None) == cpx.CPX_OK
    assert all(orc.g1_eq_jac(bytes(j)[JAC * i:JAC * (i + 1)], want[i]) for i in range(n))
    assert L.cpx_g1_msm_many(h, n, lens, bases, scalars, None, c) == cpx.CPX_OK
    assert bytes(c) == b"".join(orc.g1_compress_jac(w) for w in want)
    assert L.cpx_g1_msm_many(h, n, lens, bases, scalars, None, None) == cpx.CPX_OK


def test_msm_many_with_1_2_and_4_slices(orc, pool):
    """(1030, 5, 0, 64): 4 tasks x 16 waves leave the GPU almost empty and a quarter of 1030 points is still 257, so the call takes 4 waves
    per window; the short tasks then have slices beyond their end, the empty one nothing but such slices"""
    import curdleproofs_amd as cpx
    tasks = pool.tasks(SLICED)
    c = cpx.Context(0)
    try:
        assert c.get_option("tbw_slices") == 0
        results = {0: _check_msm_many(c, orc, pool, tasks, against_single=False)[1]}
        for pinned in (1, 2, 4):
            c.set_option("tbw_slices", pinned)
            results[pinned] = _check_msm_many(c, orc, pool, tasks, against_single=False)[1]
        assert results[0] == results[1] == results[2] == results[4]
    finally:
        c.close()


def test_msm_many_edge_operands(ctx, orc, pool):
    """tasks of 16 points each, all in one call"""
    n = 16
    P, k = _pt(pool.points, 0, n), _sc(pool.scalars, 0, n)
    minus_one = _wire(orc, [R_ - 1])
    neg = orc.g1_scale(P, minus_one)                                    # -P_i
    zero, one = _wire(orc, [0] * n), _wire(orc, [1] * n)
    pts = lambda idx, src=P: b"".join(_pt(src, i) for i in idx)
    scs = lambda idx: b"".join(_sc(k, i) for i in idx)
    ident = bytes(AFF)
    cases = {
        "zero scalars": (P, zero),
        "scalar 1": (P, one),
        "scalar r - 1": (P, minus_one * n),
        "mixed 0, 1, r - 1, random": (P, _sc(zero, 0, 4) + _sc(one, 0, 4) + minus_one * 4 + _sc(k, 12, 4)),
        "identity bases among others": (ident + _pt(P, 1, 6) + ident * 2 + _pt(P, 9, 6) + ident, k),
        "identity bases only": (ident * n, k),
        "the same point twice with the same scalar": (pts([3, 3] + list(range(2, n))), scs([5, 5] + list(range(2, n)))),
        "a point and its negative with the same scalar": (_pt(P, 4) + _pt(neg, 4) + _pt(P, 2, n - 2), scs([7, 7] + list(range(2, n)))),
        "all cancelling": (b"".join(_pt(P, i) + _pt(neg, i) for i in range(8)), b"".join(_sc(k, i) * 2 for i in range(8))),
        "all cancelling, scalar 1 and r - 1 on one point": (_pt(P, 0) * n, (_sc(one, 0) + minus_one) * 8),
    }
    names = list(cases)
    tasks = [cases[c] for c in names]
    assert all(len(b) == AFF * n and len(s) == FR * n for b, s in tasks)
    jac, comp = _check_msm_many(ctx, orc, pool, tasks)
    for c in ("zero scalars", "identity bases only", "all cancelling", "all cancelling, scalar 1 and r - 1 on one point"):
        i = names.index(c)
        assert comp[i] == IDENTITY and jac[i][96:] == bytes(48), c          # the identity in both encodings
    i = names.index("a point and its negative with the same scalar")
    assert orc.g1_eq_jac(jac[i], pool.msm(_pt(P, 2, n - 2), _sc(k, 2, n - 2)))      # the pair sums to the identity


# ---- folds ----
class Folds:
    """PL, PR and gamma per family, and the oracle's fold, for every shape — computed once for the three forms"""

    def __init__(self, orc, pool):
        self.orc = orc
        self.gammas = [_sc(pool.scalars, 900 + f) for f in range(3)]
        self.want = {}
        for half in FOLD_HALVES:
            for f in range(3):
                pl, pr = self.operands(pool, f, half)
                self.want[(f, half)] = orc.g1_fold(pl, pr, self.gammas[f])
        # edge families of 8 elements: [0] PL == PR, [1] PL the identity, [2] PR the identity, [3] both, [4] PL == -PR, [5..7] random
        P, Q = _pt(pool.points, 700, 8), _pt(pool.points, 720, 8)
        ident = bytes(AFF)
        neg_q4 = orc.g1_scale(_pt(Q, 4), _wire(orc, [R_ - 1]))
        self.edge_pl = _pt(Q, 0) + ident + _pt(P, 2) + ident + neg_q4 + _pt(P, 5, 3)
        self.edge_pr = _pt(Q, 0) + _pt(Q, 1) + ident + ident + _pt(Q, 4) + _pt(Q, 5, 3)
        self.edge_gammas = [_wire(orc, [0]), _wire(orc, [1]), _wire(orc, [R_ - 1]), _sc(pool.scalars, 950)]
        self.edge_want = [orc.g1_fold(self.edge_pl, self.edge_pr, g) for g in self.edge_gammas]
        two_q0 = orc.g1_to_affine(orc.g1_msm(_pt(Q, 0), _wire(orc, [2])))
        assert self.edge_want[0] == self.edge_pl                                          # gamma 0: PL comes back
        assert _pt(self.edge_want[1], 0) == two_q0                                        # gamma 1 on PL == PR: the closing addition doubles
        assert _pt(self.edge_want[1], 4) == ident                                         # gamma 1 on PL == -PR cancels
        assert _pt(self.edge_want[2], 0) == ident                                         # gamma r - 1 on PL == PR cancels to 96 zero bytes
        assert all(_pt(w, 3) == ident for w in self.edge_want)                            # identity on both sides
        assert all(_pt(w, 2) == _pt(P, 2) for w in self.edge_want)                        # PR the identity: PL comes back

    @staticmethod
    def operands(pool, f, half):
        return _pt(pool.points, 200 * f, half), _pt(pool.points, 200 * f + 130, half)


@pytest.fixture(scope="module")
def folds(orc, pool):
    return Folds(orc, pool)


@pytest.mark.parametrize("form", list(FORMS))
def test_fold_many_shapes_and_edge_gammas_in_every_form(orc, pool, folds, form):
    import curdleproofs_amd as cpx
    options, quad_launches = FORMS[form]
    c = cpx.Context(0, options=options)
    try:
        c.set_profiling(True)
        assert c.get_option("fold_quad_max") == options.get("fold_quad_max", 1536)
        for families in FOLD_FAMILIES:
            for half in FOLD_HALVES:
                ops = [Folds.operands(pool, f, half) for f in range(families)]
                c.reset_stats()
                got = c.fold_many([pl for pl, _ in ops], [pr for _, pr in ops], folds.gammas[:families])
                assert got == [folds.want[(f, half)] for f in range(families)], (families, half)          # byte-equal to the oracle per family
                assert c.stat("k_smul")["launches"] == 1 and c.stat("k_smul")["units"] == families * half
                assert c.stat("k_smul_quad")["launches"] == quad_launches, (families, half)
        # the gammas b"".join()ed are taken as well as the list
        c.reset_stats()
        got = c.fold_many([folds.edge_pl] * 4, [folds.edge_pr] * 4, b"".join(folds.edge_gammas))
        assert got == folds.edge_want
        assert c.stat("k_smul_quad")["launches"] == quad_launches
        if form == "default":                                   # the option moves the switch: 3 x 128 elements above a threshold of 383
            c.set_option("fold_quad_max", 383)
            for families, want_quad in ((3, 0), (2, 1)):
                ops = [Folds.operands(pool, f, 128) for f in range(families)]
                c.reset_stats()
                assert c.fold_many([pl for pl, _ in ops], [pr for _, pr in ops], folds.gammas[:families]) == [folds.want[(f, 128)] for f in range(families)]
                assert c.stat("k_smul_quad")["launches"] == want_quad
    finally:
        c.close()


# ---- a whole chain of rounds ----
def test_five_rounds_of_cross_terms_and_folds_match_the_oracle(ctx, orc, pool):
    rnd = random.Random(20261019)
    G = G_ref = _pt(pool.points, 1000, 32)
    x = [rnd.randrange(R_) for _ in range(32)]
    cross, cross_ref = [], []
    h = 32
    while h > 1:
        h //= 2
        xw = _wire(orc, x)
        x_l, x_r = _sc(xw, 0, h), _sc(xw, h, h)
        # L = msm(G_R, x_L), R = msm(G_L, x_R): same_multiscalar_argument.rs:107, :110
        cross += ctx.msm_many([_pt(G, h, h), _pt(G, 0, h)], [x_l, x_r])
        cross_ref += [orc.g1_msm(_pt(G_ref, h, h), x_l), orc.g1_msm(_pt(G_ref, 0, h), x_r)]
        gamma = rnd.randrange(1, R_)
        gw = _wire(orc, [gamma])
        x = [(x[i] + pow(gamma, -1, R_) * x[h + i]) % R_ for i in range(h)]
        G = ctx.fold_many([_pt(G, 0, h)], [_pt(G, h, h)], [gw])[0]
        G_ref = orc.g1_fold(_pt(G_ref, 0, h), _pt(G_ref, h, h), gw)
    assert len(cross) == 10 and len(G) == AFF
    for i, (a, b) in enumerate(zip(cross, cross_ref)):
        assert orc.g1_eq_jac(a, b) and orc.g1_compress_jac(a) == orc.g1_compress_jac(b), "cross term %d" % i
    assert G == G_ref


# ---- launches ----
def test_launch_counts_do_not_depend_on_the_count(orc, pool):
    import curdleproofs_amd as cpx
    names = ("k_msm_tblw<2, true>", "k_reduce_sets", "k_msm_tail", "k_finalize", "k_smul")
    c = cpx.Context(0)
    try:
        c.set_profiling(True)
        seen = {}
        for lens in ((33,), (33, 1, 0, 64, 17, 5, 128, 2, 9, 40)):
            tasks = pool.tasks(lens)
            c.reset_stats()
            c.msm_many([b for b, _ in tasks], [s for _, s in tasks], compressed=True)
            seen[len(lens)] = {k: c.stat(k)["launches"] for k in names}
            assert c.stat("k_msm_tblw<2, true>")["units"] == sum(lens)
            assert c.stat("k_msm_tail")["units"] == len(lens) and c.stat("k_finalize")["units"] == len(lens)
        assert seen[1] == seen[10] == {"k_msm_tblw<2, true>": 1, "k_reduce_sets": 1, "k_msm_tail": 1, "k_finalize": 1, "k_smul": 0}
        seen = {}
        for families in (1, 3):
            ops = [Folds.operands(pool, f, 16) for f in range(families)]
            c.reset_stats()
            c.fold_many([pl for pl, _ in ops], [pr for _, pr in ops], [_sc(pool.scalars, f) for f in range(families)])
            seen[families] = {k: c.stat(k)["launches"] for k in names}
            assert c.stat("k_smul")["units"] == 16 * families
        assert seen[1] == seen[3] == {"k_msm_tblw<2, true>": 0, "k_reduce_sets": 0, "k_msm_tail": 0, "k_finalize": 0, "k_smul": 1}
    finally:
        c.close()


# ---- conventions ----
def test_argument_conventions(ctx, pool):
    import curdleproofs_amd as cpx
    L, h = ctx._L, ctx._h
    fill = lambda size: (ctypes.c_uint8 * size)(*([0xaa] * size))
    lens = (ctypes.c_uint32 * 2)(1, 1)
    bases, scalars = cpx._in(_pt(pool.points, 0, 2)), cpx._in(_sc(pool.scalars, 0, 2))
    j, c = fill(JAC * 2), fill(48 * 2)
    assert L.cpx_g1_msm_many(h, 0, None, None, None, j, c) == cpx.CPX_OK                       # count = 0: a no-op
    assert L.cpx_g1_msm_many(h, 0, lens, bases, scalars, j, c) == cpx.CPX_OK
    assert L.cpx_g1_msm_many(h, 2, None, bases, scalars, j, c) == cpx.CPX_ERR_ARG              # a NULL input with count > 0
    assert L.cpx_g1_msm_many(h, 2, lens, None, scalars, j, c) == cpx.CPX_ERR_ARG
    assert L.cpx_g1_msm_many(h, 2, lens, bases, None, j, c) == cpx.CPX_ERR_ARG
    assert L.cpx_g1_msm_many(h, (1 << 16) + 1, lens, bases, scalars, j, c) == cpx.CPX_ERR_ARG  # more than 2^16 tasks: refused before lens is read
    big = (ctypes.c_uint32 * 2)(1 << 24, 1)
    assert L.cpx_g1_msm_many(h, 2, big, bases, scalars, j, c) == cpx.CPX_ERR_ARG               # more than 2^24 points: refused before a point is read
    assert bytes(j) == b"\xaa" * (JAC * 2) and bytes(c) == b"\xaa" * 96
    pl, pr, g = fill(AFF * 2), cpx._in(_pt(pool.points, 2, 2)), cpx._in(_sc(pool.scalars, 2, 2))
    assert L.cpx_g1_fold_many(h, 0, 2, pl, pr, g) == cpx.CPX_OK                                # families = 0 or half = 0: a no-op
    assert L.cpx_g1_fold_many(h, 2, 0, pl, pr, g) == cpx.CPX_OK
    assert L.cpx_g1_fold_many(h, 0, 0, None, None, None) == cpx.CPX_OK
    assert L.cpx_g1_fold_many(h, 2, 1, None, pr, g) == cpx.CPX_ERR_ARG                         # NULL with work to do
    assert L.cpx_g1_fold_many(h, 2, 1, pl, None, g) == cpx.CPX_ERR_ARG
    assert L.cpx_g1_fold_many(h, 2, 1, pl, pr, None) == cpx.CPX_ERR_ARG
    assert L.cpx_g1_fold_many(h, 2, (1 << 23) + 1, pl, pr, g) == cpx.CPX_ERR_ARG               # more than 2^24 elements
    assert bytes(pl) == b"\xaa" * (AFF * 2)


def test_loaded_batch_is_left_alone_and_a_fresh_context_serves_both_calls(orc, pool):
    import curdleproofs_amd as cpx
    ell = 28
    crs = orc.generate_crs_points(ell)
    inst = orc.make_instance(ell, 0, crs)
    tasks = pool.tasks((16, 17, 0, 3))
    want = [orc.g1_compress_jac(pool.msm(b, s)) for b, s in tasks]
    pl, pr, g = _pt(pool.points, 300, 16), _pt(pool.points, 400, 16), _sc(pool.scalars, 300)
    want_fold = orc.g1_fold(pl, pr, g)
    c = cpx.Context(0)
    try:
        c.set_crs(ell, crs)
        c.load_batch(*(inst[k] * 2 for k in ("vec_R", "vec_S", "vec_T", "vec_U", "M")))
        before = c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2)
        assert c.batch == 2 and before == [cpx.CPX_OK] * 2
        assert c.msm_many([b for b, _ in tasks], [s for _, s in tasks], compressed=True)[1] == want
        assert c.fold_many([pl], [pr], [g]) == [want_fold]
        assert c.batch == 2
        assert c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2) == before
    finally:
        c.close()
    fresh = cpx.Context(0)                                       # no CRS, nothing loaded
    try:
        assert fresh.msm_many([b for b, _ in tasks], [s for _, s in tasks], compressed=True)[1] == want
        assert fresh.fold_many([pl], [pr], [g]) == [want_fold]
        assert fresh.batch == 0
    finally:
        fresh.close()
