"""GPU parity of the stand-alone same-permutation prover and verifier: Context.same_perm_prove -> cpx_same_perm_prove /
cpx_same_perm_prove_rng, Context.same_perm_verify -> cpx_same_perm_verify.  Proof bytes, end states, challenges and status are compared item
by item with tests/same_perm_lib.py: the oracle's own sameperm_new on the very inputs and draws the library gets; verdicts and end states
with its sameperm_verify.  The library under test is never the source of an expected value.  Nothing is compared with a tolerance."""
import ctypes

import pytest

from tests import gprod_lib as gl, same_perm_lib as sl, stdrng_ref, strobe_ref, subarg_lib, subarg_prove_lib as sp, subarg_verify_lib as sv
from tests.subarg_lib import IPA, R_

pytestmark = pytest.mark.gpu

FR, AFF, JAC, ST = 32, 96, 144, 216
KEEP = 64 << 20
SCRATCH_BUFFERS = 35                       # include/cpx.h: 23 of the tier-0 set, 12 of the shuffle set
FIELDS = sl.FIELDS
OK_, REJ, DES = True, False, "deserialize"


@pytest.fixture(scope="module")
def ctx():
    import curdleproofs_amd as cpx
    c = cpx.Context(0)                      # no CRS, nothing loaded: neither call needs one
    yield c
    assert c.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    c.close()


def inputs(items):
    return [b"".join(i[f] for i in items) for f in FIELDS]


def run(ctx, items, draws=None, rngs=None):
    """one library call over the items (all of one shape); per item dict(ok, proof, state, challenges)"""
    ell, nb = items[0]["ell"], items[0]["nb"]
    rand = None if draws is None else b"".join(draws)
    out = ctx.same_perm_prove(ell, *inputs(items), b"".join(i["state_in"] for i in items), rand=rand, rngs=rngs, challenges=True)
    nc = sl.n_challenges(sl.log2(ell + nb)) * FR
    assert all(s is True or isinstance(s, ValueError) for s in out["status"])
    return [dict(ok=s is True, proof=out["proofs"][i], state=out["states"][ST * i:ST * (i + 1)], challenges=out["challenges"][nc * i:nc * (i + 1)])
            for i, s in enumerate(out["status"])]


_oracle = {}


def oracle(c, draws):
    key = tuple(c[f] for f in FIELDS) + (c["state_in"], draws)
    if key not in _oracle:
        _oracle[key] = sl.sp_prove(c, draws)
    return _oracle[key]


def check(ctx, items, draws, expect=None):
    """the call against the oracle, item by item; expect: per item whether a proof is meant to come out (the oracle must agree)"""
    got = run(ctx, items, draws)
    want = [oracle(c, d) for c, d in zip(items, draws)]
    for i, (g, w) in enumerate(zip(got, want)):
        for key in ("ok", "proof", "state", "challenges"):
            assert g[key] == w[key], "item %d: %s" % (i, key)
    assert [w["ok"] for w in want] == (list(expect) if expect is not None else [True] * len(items))
    return got


def three(ell, nb, base, **kw):
    """the first consistent, the second with arbitrary A and M (B is formed literally), the third consistent"""
    return [sl.sp_inputs(base + i, ell, nb, filler=bytes(range(7 * i)), **dict(dict(consistent=i != 1), **kw)) for i in range(3)]


def seeded(orc, items, base):
    return [sl.seeded_draws(orc, base + i, c["ell"], c["nb"]) for i, c in enumerate(items)]


def with_ints(orc, c, field, change):
    v = subarg_lib.to_ints(orc, c[field])
    change(v)
    return dict(c, **{field: subarg_lib.to_wire(orc, v)})


# ---- shapes ----
@pytest.mark.parametrize("ell,nb", [(1, 1), (2, 2), (1, 3), (4, 4), (8, 0), (124, 4), (252, 4)])
def test_three_distinct_items(ctx, orc, ell, nb):
    """(1, 1): n = 2, one factor, a 40-byte vec_a message; (1, 3): more blinders than factors; (8, 0): no H and no blinder vectors;
    (124, 4): one piece of vec_a, not full; (252, 4): two pieces, two factors per thread of the scan"""
    items = three(ell, nb, 1000 * ell + nb)
    check(ctx, items, seeded(orc, items, 50 + ell))


def test_every_thread_scans_several_elements(ctx, orc):
    ell, nb = 4 * sl.THREADS - 4, 4
    assert ell > 3 * sl.PIECE and ell % sl.PIECE                                            # four pieces, the last one not full
    items = [sl.sp_inputs(77, ell, nb), sl.sp_inputs(78, ell, nb, consistent=False, filler=bytes(100))]
    check(ctx, items, seeded(orc, items, 79))


def launches(ctx):
    return {k: v["launches"] for k, v in ctx.stats().items() if v["launches"]}


# Every kernel's launches in one call, as the library of the commit before the engine's sub-argument stack was split into layers made
# them: recorded by running this test's code with CPX_LIB pointing at that build.  Prover and verifier at (6, 2) with counts 1 and 5, the
# prover at (1, 1) and (2, 0), the verifier at (1, 0)
_PROVE = lambda L: {"k_finalize": 4 + L, "k_gprod_products": 1, "k_gprod_rdu": 1, "k_gprod_setup": 1, "k_loop_step": L, "k_msm_tail": 4 + L, "k_msm_tblw<2, true>": 4 + L,
                    "k_reduce_sets": 4 + L, "k_same_perm_step": 1, "k_smul": 1, "k_smul_quad": 1, "k_subarg_blinders": 1, "k_subarg_prove_setup": 1}
_VERIFY = {"k_compress": 1, "k_decompress": 3, "k_finalize": 2, "k_gprod_verify_steps": 1, "k_msm_tail": 1, "k_msm_tblw<2, true>": 1, "k_reduce_sets": 1,
           "k_same_perm_verify_step": 1, "k_same_perm_weights": 1, "k_smul": 2, "k_smul_quad": 2, "k_subarg_scalars": 1}
LAUNCHES = {("prove", 1): _PROVE(3), ("prove", 5): _PROVE(3), ("prove", (1, 1)): _PROVE(1), ("prove", (2, 0)): _PROVE(1),
            ("verify", 1): _VERIFY, ("verify", 5): _VERIFY, ("verify", (1, 0)): _VERIFY}


def test_count_1_equals_count_5_and_the_launches_depend_on_L_only(orc):
    import curdleproofs_amd as cpx
    ell, nb = 6, 2
    c = sl.sp_inputs(31, ell, nb)
    d = sl.seeded_draws(orc, 31, ell, nb)
    others = [sl.sp_inputs(35 + i, ell, nb, filler=bytes(i + 1)) for i in range(4)]
    ctx = cpx.Context(0)
    try:
        ctx.set_profiling(True)
        seen, proofs, vseen = {}, {}, {}
        for count in (1, 5):
            items = ([c] + others)[:count]
            ctx.reset_stats()
            got = check(ctx, items, [d] + seeded(orc, others, 700)[:count - 1])
            proofs[count] = got[0]
            seen[count] = {k: v["launches"] for k, v in ctx.stats().items() if v["launches"]}
            assert ctx.stat("k_same_perm_step")["units"] == count
            ctx.reset_stats()
            vcheck(ctx, orc, items, [g["proof"] for g in got], [OK_] * count)
            vseen[count] = {k: v["launches"] for k, v in ctx.stats().items() if v["launches"]}
        assert proofs[1] == proofs[5]                                          # the same bytes alone as in a call of five
        assert seen[1] == seen[5] and vseen[1] == vseen[5]
        assert all(seen[1][k] == 1 for k in ("k_same_perm_step", "k_gprod_products", "k_gprod_setup", "k_gprod_rdu", "k_subarg_blinders", "k_subarg_prove_setup"))
        assert seen[1]["k_loop_step"] == 3
        assert all(vseen[1][k] == 1 for k in ("k_same_perm_verify_step", "k_same_perm_weights", "k_gprod_verify_steps", "k_subarg_scalars"))
        table = {("prove", 1): seen[1], ("prove", 5): seen[5], ("verify", 1): vseen[1], ("verify", 5): vseen[5]}
        for shape in ((1, 1), (2, 0)):                                         # the single round of n = 2, with a blinder and without H
            it = sl.sp_inputs(41, *shape)
            ctx.reset_stats()
            check(ctx, [it], [sl.seeded_draws(orc, 41, *shape)])
            table["prove", shape] = launches(ctx)
        p = got[0]["proof"]                                                    # n = 1: no round, no H; another proof's head and finals
        ctx.reset_stats()
        vcheck(ctx, orc, [sl.sp_inputs(42, 1, 0)], [p[:HEAD + 96] + p[-64:]], [REJ])
        table["verify", (1, 0)] = launches(ctx)
        print("LAUNCHES", table)
        assert table == LAUNCHES
        assert ctx.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    finally:
        ctx.close()


# ---- the rate position ----
def test_entry_states_that_put_step_1_across_the_rate_boundary(ctx, orc):
    """the entry states of tests/test_same_perm_cpu.py: the length prefix, a scalar, the last byte and the next operation header cut by
    byte 166 of the rate, and a message that ends on it"""
    from tests.test_same_perm_cpu import boundary_cases
    cases = boundary_cases()
    assert {name for name, _, _, _ in cases} == {"prefix", "scalar", "last_byte", "header", "ends_on_boundary"}
    for ell, nb in sorted({(e, b) for _, e, b, _ in cases}):
        items = [sl.sp_inputs(680 + f, e, b, filler=bytes(f)) for _, e, b, f in cases if (e, b) == (ell, nb)]
        check(ctx, items, [sl.seeded_draws(orc, 680, ell, nb)] * len(items))


# ---- exceptional operands ----
def test_exceptional_operands(ctx, orc):
    ell, nb = 6, 2
    base = sl.sp_inputs(640, ell, nb)
    items = [base,
             dict(base, A=bytes(JAC)),                                                        # A the identity
             dict(base, M=bytes(JAC)),                                                        # M the identity: the B task has an identity base
             dict(base, A=bytes(JAC), M=bytes(JAC)),
             dict(base, G=base["G"][:2 * AFF] + bytes(AFF) + base["G"][3 * AFF:]),            # an identity base in G
             dict(base, a=bytes(ell * FR)),                                                   # vec_a all zero
             dict(base, perm=sl.perm_bytes(list(range(ell)))),                                # the identity permutation ...
             dict(base, perm=sl.perm_bytes(list(range(ell))[::-1]))]                          # ... and the reversal
    check(ctx, items, [sl.seeded_draws(orc, 642, ell, nb)] * len(items))


def test_a_repeated_permutation_entry_gets_the_oracles_bytes_and_is_rejected(ctx, orc):
    ell, nb = 6, 2
    base = sl.sp_inputs(650, ell, nb)
    p = sl.perm_list(base["perm"])
    p[3] = p[0]
    c = dict(base, perm=sl.perm_bytes(p))
    got = check(ctx, [c, base], [sl.seeded_draws(orc, 651, ell, nb)] * 2)
    vcheck(ctx, orc, [c, base], [g["proof"] for g in got], [REJ, OK_])


# ---- refused items ----
def test_refused_items_between_good_ones(ctx, orc):
    """c[n - 2] = 0 (inner_product_argument.rs:69) on the extended vector: a zero draw of vec_c_blinders"""
    ell, nb = 2, 2
    items = three(ell, nb, 5002)
    draws = seeded(orc, items, 91)
    good = check(ctx, items, draws)
    dr = draws[1][:(nb - 2) * FR] + bytes(FR) + draws[1][(nb - 1) * FR:]
    got = check(ctx, items, [draws[0], dr, draws[2]], expect=[True, False, True])
    assert got[0] == good[0] and got[2] == good[2]                                            # the neighbours are bit-exact
    L = sl.log2(ell + nb)
    assert not got[1]["ok"] and got[1]["proof"] == bytes(sl.proof_bytes(L)) and got[1]["state"] == items[1]["state_in"]
    assert got[1]["challenges"] == bytes(sl.n_challenges(L) * FR)


# ---- the _rng form ----
def _rng_seeds(draws):
    s = 2
    while True:
        m = stdrng_ref.StdRng.seed_from_u64(s)
        m.fr(draws)
        if m.word_pos > 8 * draws:
            return [0, 1, s]
        s += 1


@pytest.mark.parametrize("ell,nb", [(6, 2), (8, 0), (60, 4)])
def test_rng_form_draws_the_oracles_stream(ctx, orc, ell, nb):
    from curdleproofs_amd.rng import StdRng
    k = sl.draws_each(ell, nb)
    seeds = _rng_seeds(k)
    models = [stdrng_ref.StdRng.seed_from_u64(s) for s in seeds]
    draws = [orc.rng(s).fr(k) for s in seeds]
    assert [m.fr(k) for m in models] == draws
    items = [sl.sp_inputs(800 + i, ell, nb, filler=bytes(3 * i)) for i in range(len(seeds))]
    explicit = check(ctx, items, draws)
    rngs = [StdRng.seed_from_u64(s) for s in seeds]
    assert run(ctx, items, rngs=rngs) == explicit
    assert [r.state for r in rngs] == [m.state() for m in models]


def test_rng_streams_advance_whatever_the_status(ctx, orc):
    """A refused item of the _rng form cannot be aimed at: the reference panics on c[n - 2] = 0 or on a vanishing denominator, and with
    rngs both are draws (n_blinders >= 2) or products of factors that hang on alpha and beta, which follow vec_a (n_blinders = 1).  The
    refusal itself is covered by the explicit form above, on the same code path; here every stream of a call advances by the item's draws,
    beside an item of the explicit form that IS refused in the same shape."""
    from curdleproofs_amd.rng import StdRng
    ell, nb = 2, 2
    k = sl.draws_each(ell, nb)
    items = [sl.sp_inputs(5001, ell, nb), sl.sp_inputs(5003, ell, nb)]
    rngs = [StdRng.seed_from_u64(5), StdRng.seed_from_u64(6)]
    got = run(ctx, items, rngs=rngs)
    models = [stdrng_ref.StdRng.seed_from_u64(5), stdrng_ref.StdRng.seed_from_u64(6)]
    d = [m.fr(k) for m in models]
    assert [r.state for r in rngs] == [m.state() for m in models]
    for g, c, dd in zip(got, items, d):
        w = oracle(c, dd)
        assert g == dict(ok=True, proof=w["proof"], state=w["state"], challenges=w["challenges"])
    zero = bytes(FR) + d[0][FR:]                                                              # vec_c_blinders[0] = c[n - 2] = 0
    check(ctx, [items[0], items[1]], [zero, d[1]], expect=[False, True])


# ---- refusals ----
def test_refusals_write_nothing(ctx, orc):
    import curdleproofs_amd as cpx
    ell, nb = 3, 1
    L = 2
    c = sl.sp_inputs(41, ell, nb)
    d = sl.seeded_draws(orc, 43, ell, nb)
    nc, pb = sl.n_challenges(L) * FR, sl.proof_bytes(L)
    fill = lambda size: (ctypes.c_uint8 * size)(*([0xaa] * size))
    fns = (ctx._L.cpx_same_perm_prove, ctx._L.cpx_same_perm_prove_rng)
    rng0 = stdrng_ref.StdRng.seed_from_u64(9).state()

    def refused(code, count=1, ell=ell, nb=nb, it=None, draws=d, state=None, null=None, rng=False):
        st = (ctypes.c_uint8 * ST).from_buffer_copy(state or c["state_in"])
        proof, chal, status = fill(pb), fill(nc), (ctypes.c_int * 1)(12345)
        rs = (ctypes.c_uint8 * 40).from_buffer_copy(rng0)
        args = inputs([it or c]) + [rs if rng else draws]
        outs = [st, proof, chal, status]
        if null is not None:
            if null < len(args):
                args[null] = None
            else:
                outs[null - len(args)] = None
        assert fns[1 if rng else 0](ctx._h, count, ell, nb, *args, *outs) == code
        assert bytes(st) == (state or c["state_in"]) and bytes(proof) == b"\xaa" * pb and bytes(chal) == b"\xaa" * nc and status[0] == 12345
        assert bytes(rs) == rng0

    over = R_.to_bytes(32, "little")                                       # the limbs of r itself: not reduced
    for rng in (False, True):
        refused(cpx.CPX_ERR_ARG, it=dict(c, a=c["a"][:FR * 2] + over), rng=rng)   # an unreduced scalar in each scalar input
        refused(cpx.CPX_ERR_ARG, it=dict(c, ra=over), rng=rng)
        refused(cpx.CPX_ERR_ARG, it=dict(c, rm=over), rng=rng)
        refused(cpx.CPX_ERR_ARG, it=dict(c, perm=sl.perm_bytes([0, ell, 1])), rng=rng)          # an entry >= ell
        refused(cpx.CPX_ERR_ARG, it=dict(c, perm=sl.perm_bytes([0, 1, 0xffffffff])), rng=rng)
        w = subarg_lib.words(c["state_in"])
        refused(cpx.CPX_ERR_ARG, state=subarg_lib.state_bytes(w[:25] + [strobe_ref.RATE, w[26]]), rng=rng)      # pos = 166
        refused(cpx.CPX_ERR_ARG, ell=0, nb=4, rng=rng)                     # the reference's ell - 1 underflows
        refused(cpx.CPX_ERR_ARG, ell=1, nb=0, rng=rng)                     # n = 1: the IPA's n - 2
        for bad in ((3, 0), (2, 1), (4, 2)):
            refused(cpx.CPX_ERR_NOT_POW2, ell=bad[0], nb=bad[1], rng=rng)
        refused(cpx.CPX_ERR_ARG, count=16384 + 1, rng=rng)                 # one item over the task limit: before anything is read
        refused(cpx.CPX_ERR_ARG, count=(1 << 24) // (2 * 4096 + 2) + 1, ell=4092, nb=4, rng=rng)               # ... and over the point limit
        for hole in list(range(10)) + [10, 11, 13]:                        # every input, the states, the proofs, the status
            refused(cpx.CPX_ERR_ARG, null=hole, rng=rng)
    refused(cpx.CPX_ERR_ARG, draws=d[:FR] + over + d[2 * FR:])             # an unreduced draw
    st = (ctypes.c_uint8 * ST).from_buffer_copy(c["state_in"])
    assert fns[0](ctx._h, 0, ell, nb, *([None] * 10), st, None, None, None) == cpx.CPX_OK       # count = 0: a no-op
    assert bytes(st) == c["state_in"]
    for kw in (dict(), dict(rand=d, rngs=[])):                             # neither, both
        with pytest.raises(ValueError):
            ctx.same_perm_prove(ell, *inputs([c]), c["state_in"], **kw)
    # n_blinders = 0: H and the blinder vectors may be NULL; the challenges may be NULL; and the context still proves a good item
    c0 = sl.sp_inputs(44, 4, 0)
    d0 = sl.seeded_draws(orc, 45, 4, 0)
    args = inputs([c0]) + [d0]
    args[1] = args[7] = args[8] = None
    st, proof, status = (ctypes.c_uint8 * ST).from_buffer_copy(c0["state_in"]), fill(pb), (ctypes.c_int * 1)(12345)
    assert fns[0](ctx._h, 1, 4, 0, *args, st, proof, None, status) == cpx.CPX_OK
    w = oracle(c0, d0)
    assert status[0] == cpx.CPX_OK and bytes(st) == w["state"] and bytes(proof) == w["proof"]


# ---- isolation and regression ----
def test_loaded_batch_and_crs_are_left_alone(orc):
    import curdleproofs_amd as cpx
    ell = 28
    crs = orc.generate_crs_points(ell)
    inst = orc.make_instance(ell, 0, crs)
    c = cpx.Context(0)
    try:
        c.set_crs(ell, crs)
        c.load_batch(*(inst[k] * 2 for k in ("vec_R", "vec_S", "vec_T", "vec_U", "M")))
        before = c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2)
        assert c.batch == 2 and before == [cpx.CPX_OK] * 2
        items = [sl.sp_inputs(31, 6, 2)] * 2
        got = check(c, items, [sl.seeded_draws(orc, 31, 6, 2)] * 2)
        vcheck(c, orc, items, [g["proof"] for g in got], [OK_] * 2)
        assert c.batch == 2
        assert c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2) == before
        assert c.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    finally:
        c.close()


def test_gprod_prove_and_ipa_prove_are_undisturbed_on_the_same_context(ctx, orc):
    """the shared scratch and the shared kernels: the same cpx_ipa_prove and cpx_gprod_prove before and after a cpx_same_perm_prove and a
    cpx_same_perm_verify, against the oracle"""
    n = 8
    item = sp.sp_inputs(IPA, 901, n)
    draws = sp.seeded_draws(orc, IPA, 901, n)
    want = sp.sp_prove(item, draws)
    gc = gl.gp_inputs(902, 6, 2)
    gd = gl.seeded_draws(orc, 903, 6, 2)
    gwant = gl.gp_prove(gc, gd)
    gf = ("G", "H", "crs_U", "B", "result", "b", "rb")

    def ipa():
        out = ctx.ipa_prove(n, *item["bases"], *item["stmt"], item["z"], *item["vecs"], item["state_in"], rand=draws, challenges=True)
        return out["proofs"][0], out["states"], out["challenges"]

    def gprod():
        out = ctx.gprod_prove(6, *[gc[f] for f in gf], gc["state_in"], rand=gd, challenges=True)
        return out["proofs"][0], out["states"], out["challenges"]

    first, gfirst = ipa(), gprod()
    s = [sl.sp_inputs(904, 6, 2)]
    got = check(ctx, s, seeded(orc, s, 905))
    vcheck(ctx, orc, s, [got[0]["proof"]], [OK_])
    assert ipa() == first == (want["proof"], want["state"], want["challenges"])
    assert gprod() == gfirst == (gwant["proof"], gwant["state"], gwant["challenges"])


# ---- one large shape: the absorb is not capped by LDS ----
def test_ell_4092_round_trip(ctx, orc):
    """the consistent statement is made with the context's own MSM; the oracle's prover is not run at this size.  alpha and beta against
    tests/strobe_ref.py, then the round trip through same_perm_verify"""
    ell, nb = 4092, 4
    r = orc.rng(4092)
    G, H = r.g1_affine(ell), r.g1_affine(nb)
    U = _jac(r.g1_affine(1))
    a = r.fr(ell)
    ra, rm = r.fr(nb), r.fr(nb)
    perm = list(range(ell))
    m = stdrng_ref.StdRng.seed_from_u64(4093)
    for i in range(ell - 1, 0, -1):
        j = m.next_u32() % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    a_ints = subarg_lib.to_ints(orc, a)
    A = ctx.msm(G + H, subarg_lib.to_wire(orc, [a_ints[s] for s in perm]) + ra)
    M = ctx.msm(G + H, subarg_lib.to_wire(orc, perm) + rm)
    state_in = subarg_lib.entry_state(b"large")
    draws = sl.seeded_draws(orc, 4094, ell, nb)
    out = ctx.same_perm_prove(ell, G, H, U, A, M, a, perm, ra, rm, state_in, rand=draws, challenges=True)
    assert out["status"] == [True]
    _, alpha, beta = sl.model_step1(state_in, orc.g1_compress_jac(A), orc.g1_compress_jac(M), a_ints)
    assert subarg_lib.to_ints(orc, out["challenges"][:2 * FR]) == [alpha, beta]
    g_sum = orc.g1_to_affine(ctx.msm(G, subarg_lib.to_wire(orc, [1] * ell)))
    h_sum = orc.g1_to_affine(ctx.msm(H, subarg_lib.to_wire(orc, [1] * nb)))
    ver = ctx.same_perm_verify(ell, G, H, U, g_sum, h_sum, A, M, a, out["proofs"][0], sl.factors(orc, 4095), state_in, challenges=True)
    assert ver["verdicts"] == [True] and ver["states"] == out["states"] and ver["challenges"] == out["challenges"]
    swapped = a[FR:2 * FR] + a[:FR] + a[2 * FR:]
    assert ctx.same_perm_verify(ell, G, H, U, g_sum, h_sum, A, M, swapped, out["proofs"][0], sl.factors(orc, 4095), state_in)["verdicts"] == [False]


def _jac(aff):
    from curdleproofs_amd import params
    return aff + (bytes(48) if aff == bytes(96) else params.fp_to_wire(1))


# ---- the verifier: Context.same_perm_verify -> cpx_same_perm_verify against the oracle's sameperm_verify ----
VORDER = ("G", "H", "crs_U", "g_sum", "h_sum", "A", "M", "a")
IPA_POINTS = ("B_c", "B_d", "L_C", "R_C", "L_D", "R_D")
HEAD = 48 + 80                              # B, C, r_p ahead of the InnerProductProof's bytes


def vrun(ctx, items, proofs, rand):
    """one library call; per item dict(verdict = True / False / "deserialize", state, challenges)"""
    from curdleproofs_amd.whisk import SerializationError
    cat = lambda k: b"".join(i[k] for i in items)
    ell, nb = items[0]["ell"], items[0]["nb"]
    out = ctx.same_perm_verify(ell, *[cat(k) for k in VORDER], b"".join(proofs), rand, cat("state_in"), challenges=True)
    nc = sl.n_challenges(sl.log2(ell + nb)) * FR
    code = lambda v: DES if isinstance(v, SerializationError) else v
    return [dict(verdict=code(v), state=out["states"][ST * i:ST * (i + 1)], challenges=out["challenges"][nc * i:nc * (i + 1)]) for i, v in enumerate(out["verdicts"])]


def vcheck(ctx, orc, items, proofs, expect, seed=73):
    """the call against the oracle's verifier item by item: verdict and end state; expect: the verdicts meant (the oracle must agree)"""
    rand = sl.factors(orc, seed, len(items))
    got = vrun(ctx, items, proofs, rand)
    want = [sl.sp_verify(c, p, rand[3 * FR * i:3 * FR * (i + 1)]) for i, (c, p) in enumerate(zip(items, proofs))]
    assert [w["verdict"] for w in want] == list(expect)
    for i, (g, w, c) in enumerate(zip(got, want, items)):
        assert g["verdict"] == w["verdict"] and g["state"] == w["state"], "item %d" % i
        if w["verdict"] == DES:
            assert g["state"] == c["state_in"] and g["challenges"] == bytes(len(g["challenges"]))
    return got


@pytest.fixture(scope="module")
def proven(orc):
    """three consistent items of (6, 2) with the oracle's proofs"""
    items = [sl.sp_inputs(8100 + i, 6, 2, filler=bytes(range(7 * i))) for i in range(3)]
    return items, [oracle(c, d) for c, d in zip(items, seeded(orc, items, 81))]


def with_ipa_point(proof, slot, enc):
    return proof[:HEAD + 48 * slot] + enc + proof[HEAD + 48 * (slot + 1):]


def flip_scalar(proof, at):
    return proof[:at] + bytes([proof[at] ^ 1]) + proof[at + 1:]


@pytest.mark.parametrize("ell,nb", [(1, 1), (6, 2), (8, 0), (124, 4)])
def test_verifier_accepts_what_the_prover_makes(ctx, orc, ell, nb):
    """same_perm_prove then same_perm_verify; both leave the oracle's state and challenges"""
    items = [sl.sp_inputs(8200 + ell + i, ell, nb, filler=bytes(range(5 * i))) for i in range(3)]
    made = run(ctx, items, seeded(orc, items, 82))
    assert all(m["ok"] for m in made)
    got = vcheck(ctx, orc, items, [m["proof"] for m in made], [OK_] * 3)
    for g, m in zip(got, made):
        assert g["state"] == m["state"] and g["challenges"] == m["challenges"]


def test_verifier_rejects_a_changed_statement(ctx, orc, proven):
    items, made = proven
    c, p = items[1], made[1]["proof"]
    s = orc.rng(14).fr(1)
    a = c["a"]
    changed = [dict(c, A=orc.g1_msm(orc.g1_to_affine(c["A"]), s)),
               dict(c, M=orc.g1_msm(orc.g1_to_affine(c["M"]), s)),
               with_ints(orc, c, "a", lambda v: v.__setitem__(2, v[2] + 1)),
               dict(c, a=a[FR:2 * FR] + a[:FR] + a[2 * FR:]),                                            # two entries swapped
               dict(c, g_sum=items[0]["g_sum"])]
    vcheck(ctx, orc, changed, [p] * len(changed), [REJ] * len(changed))


def test_verifier_rejects_one_flipped_field_at_a_time(ctx, orc, proven):
    items, made = proven
    c, p, other = items[1], made[1]["proof"], made[0]["proof"]
    L = 3
    muts = [other[:48] + p[48:], p[:48] + other[48:96] + p[96:], flip_scalar(p, 96)]                     # B, C, r_p
    for name in IPA_POINTS:
        slot = sv.slot(IPA, L, name)
        muts.append(with_ipa_point(p, slot, other[HEAD + 48 * slot:HEAD + 48 * (slot + 1)]))
    muts += [flip_scalar(p, len(p) - 64), flip_scalar(p, len(p) - 32)]                                   # c_final, d_final
    assert len(set(muts)) == 11 and p not in muts
    vcheck(ctx, orc, [c] * len(muts), muts, [REJ] * len(muts))


def test_verifier_flags_what_does_not_deserialise_and_keeps_its_state(ctx, orc, proven):
    from tests import decoding_ref
    items, made = proven
    c, p = items[1], made[1]["proof"]
    outside = decoding_ref.encode(decoding_ref.non_member_points(orc, 1)[0][0], 0x80)
    off = decoding_ref.encode(decoding_ref.off_curve_xs(1)[0], 0x80)
    bad = [outside + p[48:],                                                                             # B outside the subgroup
           off + p[48:],                                                                                 # B's x not on the curve
           bytes(48) + p[48:],                                                                           # B without the compression flag
           p[:48] + outside + p[96:],                                                                    # C outside the subgroup
           p[:96] + R_.to_bytes(32, "little") + p[HEAD:],                                                # r_p = r
           with_ipa_point(p, sv.slot(IPA, 3, "R_D", 1), outside),                                        # an IPA point outside the subgroup
           p[:-32] + R_.to_bytes(32, "little")]                                                          # d_final = r
    vcheck(ctx, orc, [c] * len(bad), bad, [DES] * len(bad))


def test_verifier_mixed_verdicts_in_one_call(ctx, orc, proven):
    items, made = proven
    p = [m["proof"] for m in made]
    wrong = with_ints(orc, items[1], "a", lambda v: v.__setitem__(0, v[0] + 1))
    broken = p[2][:96] + R_.to_bytes(32, "little") + p[2][HEAD:]
    got = vcheck(ctx, orc, [items[0], wrong, items[2], items[2], items[0]], [p[0], p[1], broken, p[2], p[0]], [OK_, REJ, DES, OK_, OK_])
    alone = vcheck(ctx, orc, [items[0]], [p[0]], [OK_])                                                  # the same item alone: the same draws are its factors
    assert alone[0] == got[0]


def test_verifier_at_n_1_is_a_real_check(ctx, orc, proven):
    """n = 1: no round; the prover cannot make such a proof (its n - 2 underflows), so the bytes are another proof's head and finals"""
    _, made = proven
    p = made[0]["proof"]
    c = sl.sp_inputs(8300, 1, 0)
    vcheck(ctx, orc, [c], [p[:HEAD + 96] + p[-64:]], [REJ])


def test_the_new_relation_in_isolation(ctx, orc):
    """a proof whose grand-product relations hold on (B', product) but whose B' is not A + alpha M + beta sum G: vec_b_blinders' differs from
    r_a + alpha r_m, B' = <factors, G> + <b', H>.  gprod_verify accepts it from the state after step 1, same_perm_verify must reject it, and
    the oracle agrees with both.  A verifier that forgets the accumulate_check of same_permutation_argument.rs:149 accepts here."""
    ell, nb = 6, 2
    c = sl.sp_inputs(8400, ell, nb)
    d = sl.sp_derive(c)                                                                       # the oracle's step 1: alpha, beta, factors, the state after it
    t, alpha, beta = sl.model_step1(c["state_in"], orc.g1_compress_jac(c["A"]), orc.g1_compress_jac(c["M"]), subarg_lib.to_ints(orc, c["a"]))
    assert subarg_lib.to_ints(orc, d["alpha"] + d["beta"]) == [alpha, beta] and subarg_lib.state_bytes(t.to_words()) == d["state"]
    from curdleproofs_amd.transcript import Transcript
    st = Transcript.from_state(c["state_in"])                                                 # step 1 through the context's transcript calls
    st.append_message(b"same_perm_step1", orc.g1_compress_jac(c["A"]))
    st.append_message(b"same_perm_step1", orc.g1_compress_jac(c["M"]))
    st.append_message(b"same_perm_step1", sl.vec_a_message(subarg_lib.to_ints(orc, c["a"])))
    assert st.challenge_scalar(b"same_perm_alpha") == d["alpha"] and st.challenge_scalar(b"same_perm_beta") == d["beta"] and st.state == d["state"]
    rb = subarg_lib.to_ints(orc, d["rb"])
    rb2 = subarg_lib.to_wire(orc, [rb[0] + 1] + rb[1:])
    assert rb2 != d["rb"]
    B2 = ctx.msm(c["G"] + c["H"], d["b"] + rb2)
    draws = sl.seeded_draws(orc, 8401, ell, nb)
    out = ctx.gprod_prove(ell, c["G"], c["H"], c["crs_U"], B2, d["result"], d["b"], rb2, d["state"], rand=draws)
    assert out["status"] == [True]
    gproof = out["proofs"][0]
    assert gproof == sl.sp_gprod(c, d["state"], B2, d["result"], d["b"], rb2, draws)["proof"]
    f3 = sl.factors(orc, 8402)
    gv = ctx.gprod_verify(ell, c["G"], c["H"], c["crs_U"], c["g_sum"], c["h_sum"], B2, d["result"], gproof, f3[FR:], d["state"])
    assert gv["verdicts"] == [True]                                                           # the grand-product relations hold ...
    proof = orc.g1_compress_jac(B2) + gproof
    want = sl.sp_verify(c, proof, f3)
    assert want["verdict"] is False                                                           # ... and the oracle rejects through :149 alone
    got = vrun(ctx, [c], [proof], f3)[0]
    assert got["verdict"] is False and got["state"] == want["state"] == gv["states"]


def test_verifier_refusals_write_nothing(ctx, orc, proven):
    import curdleproofs_amd as cpx
    items, made = proven
    c, p = items[0], made[0]["proof"]
    ell, nb, L = 6, 2, 3
    nc = sl.n_challenges(L) * FR
    rand = sl.factors(orc, 75)
    fill = lambda size: (ctypes.c_uint8 * size)(*([0xaa] * size))

    def refused(code, count=1, ell=ell, nb=nb, it=None, proof=p, rand=rand, state=None, null=None):
        st = (ctypes.c_uint8 * ST).from_buffer_copy(state or c["state_in"])
        chal, ver = fill(nc), (ctypes.c_int * 1)(12345)
        args = [(it or c)[k] for k in VORDER] + [proof, rand]
        outs = [st, chal, ver]
        if null is not None:
            if null < len(args):
                args[null] = None
            else:
                outs[null - len(args)] = None
        assert ctx._L.cpx_same_perm_verify(ctx._h, count, ell, nb, *args, *outs) == code
        assert bytes(st) == (state or c["state_in"]) and bytes(chal) == b"\xaa" * nc and ver[0] == 12345

    over = R_.to_bytes(32, "little")
    refused(cpx.CPX_ERR_ARG, it=dict(c, a=c["a"][:FR] + over + c["a"][2 * FR:]))
    for k in range(3):                                                      # a zero factor, an unreduced one, in each place
        refused(cpx.CPX_ERR_ARG, rand=rand[:k * FR] + bytes(FR) + rand[(k + 1) * FR:])
        refused(cpx.CPX_ERR_ARG, rand=rand[:k * FR] + over + rand[(k + 1) * FR:])
    w = subarg_lib.words(c["state_in"])
    refused(cpx.CPX_ERR_ARG, state=subarg_lib.state_bytes(w[:25] + [strobe_ref.RATE, w[26]]))
    refused(cpx.CPX_ERR_ARG, ell=0, nb=8)
    for bad in ((3, 0), (4, 2)):
        refused(cpx.CPX_ERR_NOT_POW2, ell=bad[0], nb=bad[1])
    refused(cpx.CPX_ERR_ARG, count=65536 + 1)
    for hole in list(range(10)) + [10, 12]:                                 # every input, the states, the verdicts
        refused(cpx.CPX_ERR_ARG, null=hole)
    st = (ctypes.c_uint8 * ST).from_buffer_copy(c["state_in"])
    assert ctx._L.cpx_same_perm_verify(ctx._h, 0, ell, nb, *([None] * 10), st, None, None) == cpx.CPX_OK    # count = 0: a no-op
    assert bytes(st) == c["state_in"]
    st, ver = (ctypes.c_uint8 * ST).from_buffer_copy(c["state_in"]), (ctypes.c_int * 1)(12345)                # the challenges may be NULL
    assert ctx._L.cpx_same_perm_verify(ctx._h, 1, ell, nb, *[c[k] for k in VORDER], p, rand, st, None, ver) == cpx.CPX_OK
    assert ver[0] == cpx.CPX_OK and bytes(st) == made[0]["state"]
