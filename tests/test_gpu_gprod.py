"""GPU parity of the stand-alone grand-product prover and verifier: Context.gprod_prove -> cpx_gprod_prove / cpx_gprod_prove_rng.  Proof bytes, end
states, challenges and status are compared item by item with tests/gprod_lib.py: the oracle's own gprod_new on the very inputs and draws
the library gets.  The library under test is never the source of an expected value.  Context.gprod_verify -> cpx_gprod_verify
is compared likewise with the oracle's gprod_verify: verdicts and end states.

vec_b_blinders = -alpha (r_p and vec_d_blinders vanish) cannot be aimed at: alpha is drawn from the transcript after the blinders are
fixed.  It is not covered.  The retrying challenge is covered by tests/test_gpu_transcript.py on the same WaveStrobe."""
import ctypes

import pytest

from tests import gprod_lib as gl, stdrng_ref, strobe_ref, subarg_lib, subarg_prove_lib as sp, subarg_verify_lib as sv
from tests.subarg_lib import IPA, R_

pytestmark = pytest.mark.gpu

FR, AFF, JAC, ST = 32, 96, 144, 216
KEEP = 64 << 20
SCRATCH_BUFFERS = 35                       # include/cpx.h: 23 of the tier-0 set, 12 of the shuffle set
FIELDS = ("G", "H", "crs_U", "B", "result", "b", "rb")


@pytest.fixture(scope="module")
def ctx():
    import curdleproofs_amd as cpx
    c = cpx.Context(0)                      # no CRS, nothing loaded: the prover needs neither
    yield c
    assert c.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    c.close()


def inputs(items):
    return [b"".join(i[f] for i in items) for f in FIELDS]


def run(ctx, items, draws=None, rngs=None):
    """one library call over the items (all of one shape); per item dict(ok, proof, state, challenges)"""
    ell, nb = items[0]["ell"], items[0]["nb"]
    rand = None if draws is None else b"".join(draws)
    out = ctx.gprod_prove(ell, *inputs(items), b"".join(i["state_in"] for i in items), rand=rand, rngs=rngs, challenges=True)
    nc = gl.n_challenges(gl.log2(ell + nb)) * FR
    assert all(s is True or isinstance(s, ValueError) for s in out["status"])
    return [dict(ok=s is True, proof=out["proofs"][i], state=out["states"][ST * i:ST * (i + 1)], challenges=out["challenges"][nc * i:nc * (i + 1)])
            for i, s in enumerate(out["status"])]


_oracle = {}


def oracle(c, draws):
    key = tuple(c[f] for f in FIELDS) + (c["filler"], draws)
    if key not in _oracle:
        _oracle[key] = gl.gp_prove(c, draws)
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
    return [gl.gp_inputs(base + i, ell, nb, filler=bytes(range(7 * i)), **kw) for i in range(3)]


def seeded(orc, items, base):
    return [gl.seeded_draws(orc, base + i, c["ell"], c["nb"]) for i, c in enumerate(items)]


def with_ints(orc, c, field, change):
    v = subarg_lib.to_ints(orc, c[field])
    change(v)
    return dict(c, **{field: subarg_lib.to_wire(orc, v)})


# ---- shapes ----
@pytest.mark.parametrize("ell,nb", [(1, 1), (2, 2), (1, 3), (4, 4), (8, 0), (124, 4), (252, 4)])
def test_three_distinct_items(ctx, orc, ell, nb):
    """(1, 1): n = 2, one prefix product and empty blinder sums; (1, 3): more blinders than factors; (8, 0): no H at all; (124, 4) and
    (252, 4): the protocol's shapes, one and two factors per thread of the scan"""
    items = three(ell, nb, 1000 * ell + nb)
    check(ctx, items, seeded(orc, items, 50 + ell))


def test_every_thread_scans_several_elements(ctx, orc):
    ell, nb = 4 * gl.THREADS - 4, 4
    items = [gl.gp_inputs(77, ell, nb), gl.gp_inputs(78, ell, nb, filler=bytes(100))]
    check(ctx, items, seeded(orc, items, 79))


def launches(ctx):
    return {k: v["launches"] for k, v in ctx.stats().items() if v["launches"]}


# Every kernel's launches in one call, as the library of the commit before the engine's sub-argument stack was split into layers made
# them: recorded by running this test's code with CPX_LIB pointing at that build.  The prover at (6, 2) with counts 1 and 5 and at
# (1, 1) and (2, 0); the verifier at (6, 2) and at (1, 0)
_PROVE = lambda L: {"k_finalize": 3 + L, "k_gprod_products": 1, "k_gprod_rdu": 1, "k_gprod_setup": 1, "k_loop_step": L, "k_msm_tail": 3 + L, "k_msm_tblw<2, true>": 3 + L,
                    "k_reduce_sets": 3 + L, "k_smul": 1, "k_smul_quad": 1, "k_subarg_blinders": 1, "k_subarg_prove_setup": 1}
_VERIFY = {"k_compress": 1, "k_decompress": 2, "k_finalize": 1, "k_gprod_verify_steps": 1, "k_msm_tail": 1, "k_msm_tblw<2, true>": 1, "k_reduce_sets": 1, "k_smul": 2,
           "k_smul_quad": 2, "k_subarg_scalars": 1}
LAUNCHES = {1: _PROVE(3), 5: _PROVE(3), (1, 1): _PROVE(1), (2, 0): _PROVE(1), "verify": _VERIFY, ("verify", 1, 0): _VERIFY}


def test_count_1_equals_count_5_and_the_launches_depend_on_L_only(orc):
    import curdleproofs_amd as cpx
    ell, nb = 6, 2
    c = gl.gp_inputs(31, ell, nb)
    d = gl.seeded_draws(orc, 31, ell, nb)
    others = [gl.gp_inputs(35 + i, ell, nb, filler=bytes(i + 1)) for i in range(4)]
    ctx = cpx.Context(0)
    try:
        ctx.set_profiling(True)
        seen, proofs = {}, {}
        for count in (1, 5):
            items = ([c] + others)[:count]
            ctx.reset_stats()
            got = check(ctx, items, [d] + seeded(orc, others, 700)[:count - 1])
            proofs[count] = got[0]
            seen[count] = launches(ctx)
            assert ctx.stat("k_gprod_setup")["units"] == count
        assert proofs[1] == proofs[5]                                          # the same bytes alone as in a call of five
        assert seen[1] == seen[5]
        assert all(seen[1][k] == 1 for k in ("k_gprod_products", "k_gprod_setup", "k_gprod_rdu", "k_subarg_blinders", "k_subarg_prove_setup"))
        assert seen[1]["k_loop_step"] == 3
        for shape in ((1, 1), (2, 0)):                                         # the single round of n = 2, with a blinder and without H
            it = gl.gp_inputs(41, *shape)
            ctx.reset_stats()
            check(ctx, [it], [gl.seeded_draws(orc, 41, *shape)])
            seen[shape] = launches(ctx)
        ctx.reset_stats()
        vcheck(ctx, orc, [c], [got[0]["proof"]], [OK_])
        seen["verify"] = launches(ctx)
        p = got[0]["proof"]                                                    # n = 1: no round, no H; another proof's head and finals
        ctx.reset_stats()
        vcheck(ctx, orc, [gl.gp_inputs(42, 1, 0)], [p[:80 + 96] + p[-64:]], [REJ])
        seen["verify", 1, 0] = launches(ctx)
        print("LAUNCHES", seen)
        assert seen == LAUNCHES
        assert ctx.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    finally:
        ctx.close()


# ---- the rate position ----
def _crossings(t):
    """what of steps 1 and 2 a rate boundary cuts, read off the model's trace"""
    out = set()
    if any(size == 48 for _, size in strobe_ref.splits(t.trace, "data")):
        out.add("point")
    if strobe_ref.splits(t.trace, "scalar"):
        out.add("scalar")
    if strobe_ref.splits(t.trace, "label"):
        out.add("label")
    return out


def test_entry_states_that_put_steps_1_and_2_across_the_rate_boundary(ctx, orc):
    """filler lengths are searched in the Python model of the transcript until steps 1 and 2 have had a 48-byte encoding, a scalar and a
    label cut by byte 166 of the rate (the positions do not depend on the values absorbed); the crossings are asserted on the model"""
    ell, nb = 1, 1
    wanted = {"point", "scalar", "label"}
    found = {}
    for f in range(1, 2 * strobe_ref.RATE):
        c = gl.gp_inputs(680, ell, nb, filler=bytes(f))
        for name in _crossings(gl.model_steps(orc, c)) & wanted:
            found.setdefault(name, c)
        if len(found) == len(wanted):
            break
    assert set(found) == wanted
    items = [found[k] for k in sorted(found)]
    check(ctx, items, [gl.seeded_draws(orc, 680, ell, nb)] * len(items))


# ---- exceptional operands ----
def test_exceptional_operands(ctx, orc):
    ell, nb = 6, 2
    base = gl.gp_inputs(640, ell, nb)
    ident_g = dict(base, G=base["G"][:2 * AFF] + bytes(AFF) + base["G"][3 * AFF:])            # an identity base in G ...
    ident_h = dict(base, H=bytes(AFF) + base["H"][AFF:])                                      # ... and in H
    ident_b = dict(base, B=bytes(JAC))                                                        # B the identity
    zero_mid = with_ints(orc, base, "b", lambda v: v.__setitem__(2, 0))                       # vec_c is zero from position 3 on
    zero_res = dict(base, result=bytes(FR))                                                   # gprod_result = 0
    items = [base, ident_g, ident_h, ident_b, zero_mid, zero_res]
    c = gl.model_products(subarg_lib.to_ints(orc, zero_mid["b"]))
    assert c[2] != 0 and c[3:] == [0] * (ell - 3)
    check(ctx, items, [gl.seeded_draws(orc, 642, ell, nb)] * len(items))


# ---- refused items ----
def test_refused_items_between_good_ones(ctx, orc):
    """c[n - 2] = 0 (inner_product_argument.rs:69) on the extended vector: a zero draw of vec_c_blinders where n_blinders >= 2, a zero
    prefix product where n_blinders = 1"""
    for ell, nb in ((2, 2), (3, 1)):
        n = ell + nb
        items = three(ell, nb, 5000 + nb)
        draws = seeded(orc, items, 91)
        good = check(ctx, items, draws)
        if nb >= 2:
            it, dr = items[1], draws[1][:(nb - 2) * FR] + bytes(FR) + draws[1][(nb - 1) * FR:]
        else:
            it, dr = with_ints(orc, items[1], "b", lambda v: v.__setitem__(0, 0)), draws[1]
            assert gl.model_products(subarg_lib.to_ints(orc, it["b"]))[n - 2] == 0
        got = check(ctx, [items[0], it, items[2]], [draws[0], dr, draws[2]], expect=[True, False, True])
        assert got[0] == good[0] and got[2] == good[2]                                        # the neighbours are bit-exact
        L = gl.log2(n)
        assert not got[1]["ok"] and got[1]["proof"] == bytes(gl.proof_bytes(L)) and got[1]["state"] == it["state_in"]
        assert got[1]["challenges"] == bytes(gl.n_challenges(L) * FR)


# ---- round trip and cross-check ----
def test_the_embedded_ipa_proof_verifies_on_a_materialised_g_prime(ctx, orc):
    """the coefficient seeding against the route that does form G': G' = u o (G | H) by Context.scale, D = B + <D's scalars, G | H> by
    Context.msm, then the EXISTING Context.ipa_verify on the proof's inner-product bytes from the state after step 2"""
    ell, nb = 6, 2
    n = ell + nb
    items = three(ell, nb, 7200)
    got = check(ctx, items, seeded(orc, items, 72))
    Gs, Us, Cs, Ds, zs, us, proofs, states = [], [], [], [], [], [], [], []
    for c, g in zip(items, got):
        alpha, beta = subarg_lib.to_ints(orc, g["challenges"][:2 * FR])
        r_p = int.from_bytes(g["proof"][48:80], "little")
        m = gl.model_layer(subarg_lib.to_ints(orc, c["b"]), subarg_lib.to_ints(orc, c["rb"]), [0] * nb, subarg_lib.to_ints(orc, c["result"])[0], alpha, beta)
        GH = c["G"] + c["H"]
        u = subarg_lib.to_wire(orc, m["u"])
        assert len(ctx.scale(GH, u)) == n * AFF                                               # G' exists on this route
        D = orc.g1_add_jac(c["B"], ctx.msm(GH, subarg_lib.to_wire(orc, m["d_scalars"])))
        inner = (r_p * pow(beta, ell + 1, R_) + subarg_lib.to_ints(orc, c["result"])[0] * pow(beta, ell, R_) - 1) % R_
        t = strobe_ref.Transcript.from_words(subarg_lib.words(c["state_in"]))                 # the state the IPA starts from
        t.append_message(b"gprod_step1", orc.g1_compress_jac(c["B"]))
        t.append_scalar(b"gprod_step1", subarg_lib.to_ints(orc, c["result"])[0])
        assert t.get_and_append_challenge(b"gprod_alpha")[0] == alpha
        t.append_message(b"gprod_step2", g["proof"][:48])
        t.append_scalar(b"gprod_step2", r_p)
        assert t.get_and_append_challenge(b"gprod_beta")[0] == beta
        Gs.append(GH)
        Us.append(c["crs_U"])
        Cs.append(_jac(orc.g1_decompress(g["proof"][:48])))
        Ds.append(D)
        zs.append(subarg_lib.to_wire(orc, [inner]))
        us.append(u)
        proofs.append(g["proof"][80:])
        states.append(subarg_lib.state_bytes(t.to_words()))
    cat = b"".join
    out = ctx.ipa_verify(n, cat(Gs), cat(Us), cat(Cs), cat(Ds), cat(zs), cat(us), cat(proofs), sv.factors(orc, 73, IPA, 3), cat(states))
    assert out["verdicts"] == [True, True, True]
    assert [out["states"][ST * i:ST * (i + 1)] for i in range(3)] == [g["state"] for g in got]   # prover and verifier leave the same transcript
    for c, g in zip(items, got):                                                              # ... and the oracle's verifier accepts the whole proof
        assert gl.gp_verify(c, g["proof"], sv.factors(orc, 74, IPA, 1))["verdict"] is True


def _jac(aff):
    from curdleproofs_amd import params
    return aff + (bytes(48) if aff == bytes(96) else params.fp_to_wire(1))


# ---- the _rng form ----
def _rng_seeds(draws):
    """seeds 0 and 1, then the first seed from 2 on whose stream rejects an Fr::rand candidate within `draws` draws (chosen on the CPU)"""
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
    k = gl.draws_each(ell, nb)
    seeds = _rng_seeds(k)
    models = [stdrng_ref.StdRng.seed_from_u64(s) for s in seeds]
    draws = [orc.rng(s).fr(k) for s in seeds]
    assert [m.fr(k) for m in models] == draws                                            # the model is the oracle's stream ...
    assert any(m.word_pos > 8 * k for m in models)                                       # ... and one of them rejects a candidate
    items = [gl.gp_inputs(800 + i, ell, nb, filler=bytes(3 * i)) for i in range(len(seeds))]
    explicit = check(ctx, items, draws)
    rngs = [StdRng.seed_from_u64(s) for s in seeds]
    assert run(ctx, items, rngs=rngs) == explicit
    assert [r.state for r in rngs] == [m.state() for m in models]                        # the oracle rng's position


def test_a_refused_item_still_advances_its_rng(ctx, orc):
    from curdleproofs_amd.rng import StdRng
    ell, nb = 3, 1
    c = gl.gp_inputs(5001, ell, nb)
    bad = with_ints(orc, c, "b", lambda v: v.__setitem__(0, 0))
    rngs = [StdRng.seed_from_u64(5), StdRng.seed_from_u64(6)]
    got = run(ctx, [bad, c], rngs=rngs)
    models = [stdrng_ref.StdRng.seed_from_u64(5), stdrng_ref.StdRng.seed_from_u64(6)]
    d = [m.fr(gl.draws_each(ell, nb)) for m in models]
    assert [r.state for r in rngs] == [m.state() for m in models]
    assert not got[0]["ok"] and got[0]["state"] == bad["state_in"]
    w = oracle(c, d[1])
    assert got[1] == dict(ok=True, proof=w["proof"], state=w["state"], challenges=w["challenges"])


# ---- refusals ----
def test_refusals_write_nothing(ctx, orc):
    import curdleproofs_amd as cpx
    ell, nb = 3, 1
    L = 2
    c = gl.gp_inputs(41, ell, nb)
    d = gl.seeded_draws(orc, 43, ell, nb)
    nc, pb = gl.n_challenges(L) * FR, gl.proof_bytes(L)
    fill = lambda size: (ctypes.c_uint8 * size)(*([0xaa] * size))
    fns = (ctx._L.cpx_gprod_prove, ctx._L.cpx_gprod_prove_rng)
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
        refused(cpx.CPX_ERR_ARG, it=dict(c, result=over), rng=rng)         # an unreduced scalar in each scalar input
        refused(cpx.CPX_ERR_ARG, it=dict(c, b=c["b"][:FR * 2] + over), rng=rng)
        refused(cpx.CPX_ERR_ARG, it=dict(c, rb=over), rng=rng)
        w = subarg_lib.words(c["state_in"])
        refused(cpx.CPX_ERR_ARG, state=subarg_lib.state_bytes(w[:25] + [strobe_ref.RATE, w[26]]), rng=rng)      # pos = 166
        refused(cpx.CPX_ERR_ARG, ell=0, nb=4, rng=rng)                     # the reference's ell - 1 underflows
        refused(cpx.CPX_ERR_ARG, ell=1, nb=0, rng=rng)                     # n = 1: the IPA's n - 2
        for bad in ((3, 0), (2, 1), (4, 2)):
            refused(cpx.CPX_ERR_NOT_POW2, ell=bad[0], nb=bad[1], rng=rng)
        refused(cpx.CPX_ERR_ARG, count=16384 + 1, rng=rng)                 # one item over the task limit: before anything is read
        refused(cpx.CPX_ERR_ARG, count=(1 << 24) // (2 * 4096 + 2) + 1, ell=4092, nb=4, rng=rng)               # ... and over the point limit
        for hole in list(range(8)) + [8, 9, 11]:                           # every input, the states, the proofs, the status
            refused(cpx.CPX_ERR_ARG, null=hole, rng=rng)
    refused(cpx.CPX_ERR_ARG, draws=d[:FR] + over + d[2 * FR:])             # an unreduced draw
    st = (ctypes.c_uint8 * ST).from_buffer_copy(c["state_in"])
    assert fns[0](ctx._h, 0, ell, nb, *([None] * 8), st, None, None, None) == cpx.CPX_OK       # count = 0: a no-op
    assert bytes(st) == c["state_in"]
    for kw in (dict(), dict(rand=d, rngs=[])):                             # neither, both
        with pytest.raises(ValueError):
            ctx.gprod_prove(ell, *inputs([c]), c["state_in"], **kw)
    # n_blinders = 0: H and vec_b_blinders may be NULL; the challenges may be NULL; and the context still proves a good item
    c0 = gl.gp_inputs(44, 4, 0)
    d0 = gl.seeded_draws(orc, 45, 4, 0)
    args = inputs([c0]) + [d0]
    args[1] = args[6] = None
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
        items = [gl.gp_inputs(31, 6, 2)] * 2
        check(c, items, [gl.seeded_draws(orc, 31, 6, 2)] * 2)
        assert c.batch == 2
        assert c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2) == before
        assert c.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    finally:
        c.close()


def test_ipa_prove_is_undisturbed_by_a_gprod_prove_on_the_same_context(ctx, orc):
    """the shared scratch and the shared setup kernel: the same cpx_ipa_prove before and after a cpx_gprod_prove, against the oracle"""
    n = 8
    item = sp.sp_inputs(IPA, 901, n)
    draws = sp.seeded_draws(orc, IPA, 901, n)
    want = sp.sp_prove(item, draws)

    def ipa():
        out = ctx.ipa_prove(n, *item["bases"], *item["stmt"], item["z"], *item["vecs"], item["state_in"], rand=draws, challenges=True)
        return out["proofs"][0], out["states"], out["challenges"]

    first = ipa()
    g = [gl.gp_inputs(902, 6, 2)]
    check(ctx, g, seeded(orc, g, 903))
    assert ipa() == first == (want["proof"], want["state"], want["challenges"])


# ---- the verifier: Context.gprod_verify -> cpx_gprod_verify against the oracle's gprod_verify ----
OK_, REJ, DES = True, False, "deserialize"
IPA_POINTS = ("B_c", "B_d", "L_C", "R_C", "L_D", "R_D")


def vrun(ctx, items, proofs, rand):
    """one library call; per item dict(verdict = True / False / "deserialize", state, challenges)"""
    from curdleproofs_amd.whisk import SerializationError
    cat = lambda k: b"".join(i[k] for i in items)
    ell, nb = items[0]["ell"], items[0]["nb"]
    out = ctx.gprod_verify(ell, cat("G"), cat("H"), cat("crs_U"), cat("g_sum"), cat("h_sum"), cat("B"), cat("result"), b"".join(proofs), rand, cat("state_in"),
                           challenges=True)
    nc = gl.n_challenges(gl.log2(ell + nb)) * FR
    code = lambda v: DES if isinstance(v, SerializationError) else v
    return [dict(verdict=code(v), state=out["states"][ST * i:ST * (i + 1)], challenges=out["challenges"][nc * i:nc * (i + 1)]) for i, v in enumerate(out["verdicts"])]


def vcheck(ctx, orc, items, proofs, expect, seed=73):
    """the call against the oracle's verifier item by item: verdict and end state; expect: the verdicts meant (the oracle must agree)"""
    rand = sv.factors(orc, seed, IPA, len(items))
    got = vrun(ctx, items, proofs, rand)
    want = [gl.gp_verify(c, p, rand[2 * FR * i:2 * FR * (i + 1)]) for i, (c, p) in enumerate(zip(items, proofs))]
    assert [w["verdict"] for w in want] == list(expect)
    for i, (g, w, c) in enumerate(zip(got, want, items)):
        assert g["verdict"] == w["verdict"] and g["state"] == w["state"], "item %d" % i
        if w["verdict"] == DES:
            assert g["state"] == c["state_in"] and g["challenges"] == bytes(len(g["challenges"]))
    return got


@pytest.fixture(scope="module")
def proven(orc):
    """three consistent items of (6, 2) with the oracle's proofs"""
    items = three(6, 2, 8100)
    return items, [oracle(c, d) for c, d in zip(items, seeded(orc, items, 81))]


def _ipa_slot(L, name, j=0):
    return sv.slot(IPA, L, name, j)


def with_ipa_point(proof, slot, enc):
    return proof[:80 + 48 * slot] + enc + proof[80 + 48 * (slot + 1):]


def flip_scalar(proof, at):
    """bit 0 of the 32-byte little-endian scalar at byte `at` (the value stays below r)"""
    return proof[:at] + bytes([proof[at] ^ 1]) + proof[at + 1:]


@pytest.mark.parametrize("ell,nb", [(1, 1), (6, 2), (8, 0), (124, 4)])
def test_verifier_accepts_what_the_prover_makes(ctx, orc, ell, nb):
    """gprod_prove then gprod_verify; both leave the oracle's state and challenges"""
    items = three(ell, nb, 8200 + ell)
    made = run(ctx, items, seeded(orc, items, 82))
    assert all(m["ok"] for m in made)
    got = vcheck(ctx, orc, items, [m["proof"] for m in made], [OK_] * 3)
    for g, m in zip(got, made):
        assert g["state"] == m["state"] and g["challenges"] == m["challenges"]


def test_verifier_rejects_a_changed_statement(ctx, orc, proven):
    """gprod_result + 1 and B * s as the reference's own test (grand_product_argument.rs:330-366); the sums are taken from the caller"""
    items, made = proven
    c, p = items[1], made[1]["proof"]
    s = orc.rng(14).fr(1)
    changed = [dict(c, result=subarg_lib.to_wire(orc, [subarg_lib.to_ints(orc, c["result"])[0] + 1])),
               dict(c, B=orc.g1_msm(orc.g1_to_affine(c["B"]), s)),
               dict(c, g_sum=items[0]["g_sum"]),
               dict(c, h_sum=items[0]["h_sum"])]
    vcheck(ctx, orc, changed, [p] * 4, [REJ] * 4)


def test_verifier_rejects_one_flipped_field_at_a_time(ctx, orc, proven):
    items, made = proven
    c, p, other = items[1], made[1]["proof"], made[0]["proof"]
    L = 3
    muts = [other[:48] + p[48:], flip_scalar(p, 48)]                                                     # C, r_p
    for name in IPA_POINTS:
        slot = _ipa_slot(L, name)
        muts.append(with_ipa_point(p, slot, other[80 + 48 * slot:80 + 48 * (slot + 1)]))
    muts += [flip_scalar(p, len(p) - 64), flip_scalar(p, len(p) - 32)]                                   # c_final, d_final
    assert len(set(muts)) == 10 and p not in muts
    vcheck(ctx, orc, [c] * len(muts), muts, [REJ] * len(muts))


def test_verifier_flags_what_does_not_deserialise_and_keeps_its_state(ctx, orc, proven):
    from tests import decoding_ref
    items, made = proven
    c, p = items[1], made[1]["proof"]
    outside = decoding_ref.encode(decoding_ref.non_member_points(orc, 1)[0][0], 0x80)
    off = decoding_ref.encode(decoding_ref.off_curve_xs(1)[0], 0x80)
    bad = [p[:48] + R_.to_bytes(32, "little") + p[80:],                                                  # r_p = r
           outside + p[48:],                                                                             # C outside the subgroup
           off + p[48:],                                                                                 # C's x not on the curve
           with_ipa_point(p, _ipa_slot(3, "R_D", 1), outside),                                           # an IPA point outside the subgroup
           p[:-32] + R_.to_bytes(32, "little")]                                                          # d_final = r
    vcheck(ctx, orc, [c] * len(bad), bad, [DES] * len(bad))


def test_verifier_mixed_verdicts_in_one_call(ctx, orc, proven):
    items, made = proven
    p = [m["proof"] for m in made]
    wrong = dict(items[1], result=subarg_lib.to_wire(orc, [subarg_lib.to_ints(orc, items[1]["result"])[0] + 1]))
    broken = p[2][:48] + R_.to_bytes(32, "little") + p[2][80:]
    got = vcheck(ctx, orc, [items[0], wrong, items[2], items[2], items[0]], [p[0], p[1], broken, p[2], p[0]], [OK_, REJ, DES, OK_, OK_])
    assert got[0] == got[4]
    alone = vcheck(ctx, orc, [items[0]], [p[0]], [OK_])                                                  # the same item alone: the same draws are its factors
    assert alone[0] == got[0]


def test_verifier_at_n_1_is_a_real_check(ctx, orc, proven):
    """n = 1: no round; the prover cannot make such a proof (its n - 2 underflows), so the bytes are another proof's head and finals"""
    _, made = proven
    p = made[0]["proof"]
    c = gl.gp_inputs(8300, 1, 0)
    vcheck(ctx, orc, [c], [p[:80 + 96] + p[-64:]], [REJ])


def test_verifier_refusals_write_nothing(ctx, orc, proven):
    import curdleproofs_amd as cpx
    items, made = proven
    c, p = items[0], made[0]["proof"]
    ell, nb, L = 6, 2, 3
    nc = gl.n_challenges(L) * FR
    rand = sv.factors(orc, 75, IPA, 1)
    fill = lambda size: (ctypes.c_uint8 * size)(*([0xaa] * size))
    order = ("G", "H", "crs_U", "g_sum", "h_sum", "B", "result")

    def refused(code, count=1, ell=ell, nb=nb, it=None, proof=p, rand=rand, state=None, null=None):
        st = (ctypes.c_uint8 * ST).from_buffer_copy(state or c["state_in"])
        chal, ver = fill(nc), (ctypes.c_int * 1)(12345)
        args = [(it or c)[k] for k in order] + [proof, rand]
        outs = [st, chal, ver]
        if null is not None:
            if null < len(args):
                args[null] = None
            else:
                outs[null - len(args)] = None
        assert ctx._L.cpx_gprod_verify(ctx._h, count, ell, nb, *args, *outs) == code
        assert bytes(st) == (state or c["state_in"]) and bytes(chal) == b"\xaa" * nc and ver[0] == 12345

    over = R_.to_bytes(32, "little")
    refused(cpx.CPX_ERR_ARG, it=dict(c, result=over))
    refused(cpx.CPX_ERR_ARG, rand=bytes(FR) + rand[FR:])                    # a zero factor
    refused(cpx.CPX_ERR_ARG, rand=rand[:FR] + over)
    w = subarg_lib.words(c["state_in"])
    refused(cpx.CPX_ERR_ARG, state=subarg_lib.state_bytes(w[:25] + [strobe_ref.RATE, w[26]]))
    refused(cpx.CPX_ERR_ARG, ell=0, nb=8)
    for bad in ((3, 0), (4, 2)):
        refused(cpx.CPX_ERR_NOT_POW2, ell=bad[0], nb=bad[1])
    refused(cpx.CPX_ERR_ARG, count=65536 + 1)
    for hole in list(range(9)) + [9, 11]:                                   # every input, the states, the verdicts
        refused(cpx.CPX_ERR_ARG, null=hole)
    st = (ctypes.c_uint8 * ST).from_buffer_copy(c["state_in"])
    assert ctx._L.cpx_gprod_verify(ctx._h, 0, ell, nb, *([None] * 9), st, None, None) == cpx.CPX_OK    # count = 0: a no-op
    assert bytes(st) == c["state_in"]
    st, ver = (ctypes.c_uint8 * ST).from_buffer_copy(c["state_in"]), (ctypes.c_int * 1)(12345)           # the challenges may be NULL
    assert ctx._L.cpx_gprod_verify(ctx._h, 1, ell, nb, *[c[k] for k in order], p, rand, st, None, ver) == cpx.CPX_OK
    assert ver[0] == cpx.CPX_OK and bytes(st) == made[0]["state"]
