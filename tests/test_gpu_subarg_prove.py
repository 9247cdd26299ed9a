"""GPU parity of the stand-alone sub-argument provers: Context.ipa_prove -> cpx_ipa_prove / cpx_ipa_prove_rng, Context.same_msm_prove ->
cpx_same_msm_prove / cpx_same_msm_prove_rng.  Proof bytes, end states, challenges and status are compared item by item with
tests/subarg_prove_lib.py: the oracle's own ipa_new / samemsm_new on the very inputs and draws the library gets.  The library under test
is never the source of an expected value.

The retrying challenge is covered by tests/test_gpu_transcript.py on the same WaveStrobe and is not repeated."""
import ctypes

import pytest

from tests import stdrng_ref, strobe_ref, subarg_lib, subarg_prove_lib as sp, subarg_verify_lib as sv
from tests.subarg_lib import IPA, SMSM, R_

pytestmark = pytest.mark.gpu

FR, AFF, JAC, ST = 32, 96, 144, 216
KINDS = pytest.mark.parametrize("kind", [IPA, SMSM], ids=["ipa", "same_msm"])
KEEP = 64 << 20
SCRATCH_BUFFERS = 35                       # include/cpx.h: 23 of the tier-0 set, 12 of the shuffle set


@pytest.fixture(scope="module")
def ctx():
    import curdleproofs_amd as cpx
    c = cpx.Context(0)                      # no CRS, nothing loaded: the provers need neither
    yield c
    assert c.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    c.close()


def inputs(kind, items):
    cat = lambda f: b"".join(f(i) for i in items)
    pts = [cat(lambda i, k=k: i["bases"][k]) for k in range(sp.FAMILIES[kind])]
    stmt = [cat(lambda i, k=k: i["stmt"][k]) for k in range(3)]
    vecs = [cat(lambda i, k=k: i["vecs"][k]) for k in range(sp.NVEC[kind])]
    return pts, stmt, cat(lambda i: i["z"]), vecs, cat(lambda i: i["state_in"])


def run(ctx, kind, n, items, draws=None, rngs=None):
    """one library call over the items; per item dict(ok, proof, state, challenges)"""
    pts, stmt, z, vecs, states = inputs(kind, items)
    rand = None if draws is None else b"".join(draws)
    if kind == IPA:
        out = ctx.ipa_prove(n, *pts, *stmt, z, *vecs, states, rand=rand, rngs=rngs, challenges=True)
    else:
        out = ctx.same_msm_prove(n, *pts, *stmt, *vecs, states, rand=rand, rngs=rngs, challenges=True)
    nc = sv.n_challenges(kind, sv.log2(n)) * FR
    assert all(s is True or isinstance(s, ValueError) for s in out["status"])
    return [dict(ok=s is True, proof=out["proofs"][i], state=out["states"][ST * i:ST * (i + 1)], challenges=out["challenges"][nc * i:nc * (i + 1)])
            for i, s in enumerate(out["status"])]


_oracle = {}


def oracle(c, draws):
    key = (c["kind"], c["n"], c["filler"], c["bases"], c["stmt"], c["z"], c["vecs"], draws)
    if key not in _oracle:
        _oracle[key] = sp.sp_prove(c, draws)
    return _oracle[key]


def check(ctx, orc, kind, n, items, draws, expect=None):
    """the call against the oracle, item by item; expect: per item whether a proof is meant to come out (the oracle must agree)"""
    got = run(ctx, kind, n, items, draws)
    want = [oracle(c, d) for c, d in zip(items, draws)]
    for i, (g, w) in enumerate(zip(got, want)):
        for key in ("ok", "proof", "state", "challenges"):
            assert g[key] == w[key], "item %d: %s" % (i, key)
    assert [w["ok"] for w in want] == (list(expect) if expect is not None else [True] * len(items))
    return got


def three(kind, n, base, **kw):
    return [sp.sp_inputs(kind, base + i, n, filler=bytes(range(7 * i)), **kw) for i in range(3)]


def seeded(orc, kind, n, items, base):
    return [sp.seeded_draws(orc, kind, base + i, n) for i in range(len(items))]


# ---- shapes ----
@pytest.mark.parametrize("kind,n", [(IPA, 2), (IPA, 4), (IPA, 8), (SMSM, 1), (SMSM, 2), (SMSM, 4), (SMSM, 8)])
def test_three_distinct_items(ctx, orc, kind, n):
    """n = 2: the blinder sums are empty; n = 8: three rounds; SameMSM n = 1: no round at all"""
    items = three(kind, n, 1000 * n + 100 * kind)
    check(ctx, orc, kind, n, items, seeded(orc, kind, n, items, 50 + n))


@pytest.mark.parametrize("n", [64, 256])     # a row one wave wide; more elements than the work-group has threads
@KINDS
def test_rows_wider_than_a_wave_and_than_the_group(ctx, orc, kind, n):
    items = [sp.sp_inputs(kind, 3 * n + kind, n), sp.sp_inputs(kind, 3 * n + kind + 7, n, filler=bytes(100))]
    check(ctx, orc, kind, n, items, seeded(orc, kind, n, items, 60 + n))


# Every kernel's launches in one call, as the library of the commit before the engine's sub-argument stack was split into layers made
# them: recorded by running this test's code with CPX_LIB pointing at that build.  n = 8 at counts 1 and 5; "small": IPA n = 2, SameMSM n = 1
_IPA_8 = {"k_finalize": 4, "k_loop_step": 3, "k_msm_tail": 4, "k_msm_tblw<2, true>": 4, "k_reduce_sets": 4, "k_smul": 1, "k_smul_quad": 1, "k_subarg_blinders": 1,
          "k_subarg_prove_setup": 1}
_SMSM_8 = {"k_compress": 1, "k_finalize": 4, "k_loop_step": 3, "k_msm_tail": 4, "k_msm_tblw<2, true>": 4, "k_reduce_sets": 4, "k_subarg_prove_setup": 1}
LAUNCHES = {
    IPA: {1: _IPA_8, 5: _IPA_8,
          "small": {"k_finalize": 2, "k_loop_step": 1, "k_msm_tail": 2, "k_msm_tblw<2, true>": 2, "k_reduce_sets": 2, "k_smul": 1, "k_smul_quad": 1, "k_subarg_blinders": 1,
                    "k_subarg_prove_setup": 1}},
    SMSM: {1: _SMSM_8, 5: _SMSM_8,
           "small": {"k_compress": 1, "k_finalize": 1, "k_msm_tail": 1, "k_msm_tblw<2, true>": 1, "k_reduce_sets": 1, "k_subarg_prove_setup": 1}},
}


@KINDS
def test_count_1_equals_count_5_and_the_launches_depend_on_L_only(orc, kind):
    import curdleproofs_amd as cpx
    n = 8
    c = sp.sp_inputs(kind, 31 + kind, n)
    d = sp.seeded_draws(orc, kind, 31 + kind, n)
    others = [sp.sp_inputs(kind, 35 + kind + i, n, filler=bytes(i + 1)) for i in range(4)]
    ctx = cpx.Context(0)
    try:
        ctx.set_profiling(True)
        seen, proofs = {}, {}
        for count in (1, 5):
            items = ([c] + others)[:count]
            ctx.reset_stats()
            got = check(ctx, orc, kind, n, items, [d] + seeded(orc, kind, n, others, 700)[:count - 1])
            proofs[count] = got[0]
            seen[count] = {k: v["launches"] for k, v in ctx.stats().items() if v["launches"]}
            assert ctx.stat("k_subarg_prove_setup")["units"] == count
        assert proofs[1] == proofs[5]                                          # the same bytes alone as in a call of five
        assert seen[1] == seen[5]
        assert seen[1]["k_subarg_prove_setup"] == 1 and seen[1]["k_loop_step"] == 3 and seen[1].get("k_subarg_blinders", 0) == (1 if kind == IPA else 0)
        m = 2 if kind == IPA else 1                                            # the single round of n = 2; n = 1: no round at all
        ctx.reset_stats()
        check(ctx, orc, kind, m, [sp.sp_inputs(kind, 41 + kind, m)], [sp.seeded_draws(orc, kind, 41 + kind, m)])
        seen["small"] = {k: v["launches"] for k, v in ctx.stats().items() if v["launches"]}
        print("LAUNCHES", kind, seen)
        assert seen == LAUNCHES[kind]
        assert ctx.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    finally:
        ctx.close()


# ---- the rate position ----
def _crossings(kind, t, n):
    """what of step 1 a rate boundary cuts, read off the model's trace"""
    out = set()
    data = strobe_ref.splits(t.trace, "data")
    if any(size == 48 for _, size in data):
        out.add("point")
    if strobe_ref.splits(t.trace, "scalar"):
        out.add("scalar")
    if strobe_ref.splits(t.trace, "label"):
        out.add("label")
    if any(size == 8 + 48 * n and k < 8 for k, size in data):
        out.add("length header")
    return out


@KINDS
def test_entry_states_that_put_step_1_across_the_rate_boundary(ctx, orc, kind):
    """filler lengths are searched in the Python model of the transcript until step 1 has had a 48-byte encoding, (IPA) the scalar z,
    a label and (SameMSM) the length header of vec_T / vec_U cut by byte 166 of the rate; the crossings are asserted on the model"""
    n = 2
    wanted = {"point", "label", "scalar" if kind == IPA else "length header"}
    found = {}
    for f in range(1, 2 * strobe_ref.RATE):
        c = sp.sp_inputs(kind, 680 + kind, n, filler=bytes(f))
        for name in _crossings(kind, sp.model_step1(orc, c, bytes(48 * sv.FIRST[kind])), n) & wanted:
            found.setdefault(name, c)
        if len(found) == len(wanted):
            break
    assert set(found) == wanted
    for name, c in found.items():
        assert name in _crossings(kind, sp.model_step1(orc, c, bytes(48 * sv.FIRST[kind])), n)
    items = [found[k] for k in sorted(found)]
    check(ctx, orc, kind, n, items, [sp.seeded_draws(orc, kind, 680 + kind, n)] * len(items))


# ---- exceptional operands ----
def _identity_jac():
    return bytes(JAC)


def _rescaled(orc, jac):
    """another representative of the same point: (X, Y, Z) -> (l^2 X, l^3 Y, l Z) with l = Z, on the field's Montgomery wire form"""
    x, y, z = jac[:48], jac[48:96], jac[96:144]
    l2 = orc.fp_mul(z, z)
    return orc.fp_mul(x, l2) + orc.fp_mul(y, orc.fp_mul(l2, z)) + orc.fp_mul(z, z)


@KINDS
def test_exceptional_operands(ctx, orc, kind):
    n = 4
    tails = sp.sp_inputs(kind, 640 + kind, n, pad=2)                                      # identity tails of G' / T / U
    base = sp.sp_inputs(kind, 641 + kind, n)
    ident = dict(base, stmt=(base["stmt"][0], _identity_jac(), base["stmt"][2]))          # a statement point that is the identity
    other = dict(base, stmt=(base["stmt"][0], base["stmt"][1], _rescaled(orc, base["stmt"][2])))   # a non-normalised representative
    assert other["stmt"][2] != base["stmt"][2] and orc.g1_eq_jac(other["stmt"][2], base["stmt"][2])
    d = sp.seeded_draws(orc, kind, 642, n)
    items = [tails, ident, other, base]
    if kind == IPA:
        items.append(dict(base, stmt=(_identity_jac(),) + base["stmt"][1:]))              # crs_H the identity
        zero_z = d[:n * FR] + bytes((n - 2) * FR)                                         # zero z draws (zero r draws: the refused case)
        draws = [d, d, d, d, d]
        items.append(base)
        draws.append(zero_z)
    else:
        items.append(dict(base, vecs=(bytes(n * FR),)))                                   # an all-zero witness
        draws = [d, d, d, d, d]
        items.append(base)
        draws.append(bytes(n * FR))                                                       # zero draws
    got = check(ctx, orc, kind, n, items, draws)
    assert got[2] == got[3]                                                               # the representative does not show in the bytes


# ---- refused IPA items ----
def test_refused_ipa_items_between_good_ones(ctx, orc):
    n = 4
    items = three(IPA, n, 5000)
    draws = seeded(orc, IPA, n, items, 91)
    good = check(ctx, orc, IPA, n, items, draws)
    # c[n-2] = 0
    c = subarg_lib.to_ints(orc, items[1]["vecs"][0])
    c[n - 2] = 0
    zero_c = dict(items[1], vecs=(subarg_lib.to_wire(orc, c), items[1]["vecs"][1]))
    # the zero denominator: r[n-1] = r[n-2] c[n-1] / c[n-2]
    c = subarg_lib.to_ints(orc, items[1]["vecs"][0])
    r = subarg_lib.to_ints(orc, draws[1])
    r[n - 1] = r[n - 2] * c[n - 1] * pow(c[n - 2], R_ - 2, R_) % R_
    zero_den = subarg_lib.to_wire(orc, r)
    nc = sv.n_challenges(IPA, sv.log2(n)) * FR
    for it, dr in ((zero_c, draws[1]), (items[1], zero_den)):
        got = check(ctx, orc, IPA, n, [items[0], it, items[2]], [draws[0], dr, draws[2]], expect=[True, False, True])
        assert got[0] == good[0] and got[2] == good[2]                                    # the neighbours are bit-exact
        assert not got[1]["ok"] and got[1]["proof"] == bytes(sv.proof_bytes(IPA, sv.log2(n))) and got[1]["state"] == it["state_in"]
        assert got[1]["challenges"] == bytes(nc)


# ---- round trip ----
@KINDS
def test_proofs_of_consistent_statements_verify_and_a_changed_witness_does_not(ctx, orc, kind):
    n = 8
    items = three(kind, n, 7200 + 10 * kind, consistent=True)
    bad = dict(items[1])
    v = subarg_lib.to_ints(orc, bad["vecs"][0])
    v[3] ^= 1                                                                             # one bit of the witness
    bad["vecs"] = (subarg_lib.to_wire(orc, v),) + bad["vecs"][1:]
    items = [items[0], bad, items[2]]
    got = check(ctx, orc, kind, n, items, seeded(orc, kind, n, items, 72))
    rand = sv.factors(orc, 73, kind, 3)
    cat = lambda f: b"".join(f(i) for i in items)
    stmt = [cat(lambda i, k=k: i["stmt"][k]) for k in range(3)]
    proofs, states = b"".join(g["proof"] for g in got), cat(lambda i: i["state_in"])
    if kind == IPA:
        out = ctx.ipa_verify(n, cat(lambda i: i["bases"][0]), *stmt, cat(lambda i: i["z"]), cat(lambda i: i["vec_u"]), proofs, rand, states)
    else:
        out = ctx.same_msm_verify(n, *[cat(lambda i, k=k: i["bases"][k]) for k in range(3)], *stmt, proofs, rand, states)
    assert out["verdicts"] == [True, False, True]
    k = sv.CHECKS[kind] * FR
    for i, (c, g) in enumerate(zip(items, got)):
        vc = dict(c, bases=c["bases"][:1] if kind == IPA else c["bases"], proof=g["proof"])
        w = sv.verify(vc, rand[k * i:k * (i + 1)])
        assert w["verdict"] == (sv.ERR_VERIFY if i == 1 else sv.OK)
        assert w["state"] == g["state"] == out["states"][ST * i:ST * (i + 1)]             # prover and verifier leave the same transcript


# ---- the _rng forms ----
def _rng_seeds(draws):
    """seeds 0 and 1, then the first seed from 2 on whose stream rejects an Fr::rand candidate within `draws` draws (chosen on the CPU)"""
    s = 2
    while True:
        m = stdrng_ref.StdRng.seed_from_u64(s)
        m.fr(draws)
        if m.word_pos > 8 * draws:
            return [0, 1, s]
        s += 1


@pytest.mark.parametrize("n", [8, 64])
@KINDS
def test_rng_forms_draw_the_oracles_stream(ctx, orc, kind, n):
    from curdleproofs_amd.rng import StdRng
    k = sp.draws_each(kind, n)
    seeds = _rng_seeds(k)
    models = [stdrng_ref.StdRng.seed_from_u64(s) for s in seeds]
    draws = [orc.rng(s).fr(k) for s in seeds]
    assert [m.fr(k) for m in models] == draws                                            # the model is the oracle's stream ...
    assert any(m.word_pos > 8 * k for m in models)                                       # ... and one of them rejects a candidate
    items = [sp.sp_inputs(kind, 800 + kind + i, n, filler=bytes(3 * i)) for i in range(len(seeds))]
    explicit = check(ctx, orc, kind, n, items, draws)
    rngs = [StdRng.seed_from_u64(s) for s in seeds]
    assert run(ctx, kind, n, items, rngs=rngs) == explicit
    assert [r.state for r in rngs] == [m.state() for m in models]                        # the oracle rng's position


def test_a_refused_item_still_advances_its_rng(ctx, orc):
    from curdleproofs_amd.rng import StdRng
    n = 4
    c = sp.sp_inputs(IPA, 5001, n)
    v = subarg_lib.to_ints(orc, c["vecs"][0])
    v[n - 2] = 0
    bad = dict(c, vecs=(subarg_lib.to_wire(orc, v), c["vecs"][1]))
    rngs = [StdRng.seed_from_u64(5), StdRng.seed_from_u64(6)]
    got = run(ctx, IPA, n, [bad, c], rngs=rngs)
    models = [stdrng_ref.StdRng.seed_from_u64(5), stdrng_ref.StdRng.seed_from_u64(6)]
    d = [m.fr(2 * n - 2) for m in models]
    assert [r.state for r in rngs] == [m.state() for m in models]
    assert not got[0]["ok"] and got[0]["state"] == bad["state_in"]
    w = oracle(c, d[1])
    assert got[1] == dict(ok=True, proof=w["proof"], state=w["state"], challenges=w["challenges"])


# ---- refusals ----
@KINDS
def test_refusals_write_nothing(ctx, orc, kind):
    import curdleproofs_amd as cpx
    n, L = 4, 2
    c = sp.sp_inputs(kind, 41 + kind, n)
    d = sp.seeded_draws(orc, kind, 43, n)
    nc, pb = sv.n_challenges(kind, L) * FR, sv.proof_bytes(kind, L)
    fill = lambda size: (ctypes.c_uint8 * size)(*([0xaa] * size))
    fns = (ctx._L.cpx_ipa_prove, ctx._L.cpx_ipa_prove_rng) if kind == IPA else (ctx._L.cpx_same_msm_prove, ctx._L.cpx_same_msm_prove_rng)
    rng0 = stdrng_ref.StdRng.seed_from_u64(9).state()

    def args_of(it, draws):
        pts, stmt, z, vecs, _ = inputs(kind, [it])
        return pts + stmt + ([z] if kind == IPA else []) + vecs + [draws]

    def refused(code, count=1, n=n, it=None, draws=d, state=None, null=None, rng=False):
        st = (ctypes.c_uint8 * ST).from_buffer_copy(state or c["state_in"])
        proof, chal, status = fill(pb), fill(nc), (ctypes.c_int * 1)(12345)
        rs = (ctypes.c_uint8 * 40).from_buffer_copy(rng0)
        args = args_of(it or c, rs if rng else draws)
        outs = [st, proof, chal, status]
        if null is not None:
            if null < len(args):
                args[null] = None
            else:
                outs[null - len(args)] = None
        assert fns[1 if rng else 0](ctx._h, count, n, *args, *outs) == code
        assert bytes(st) == (state or c["state_in"]) and bytes(proof) == b"\xaa" * pb and bytes(chal) == b"\xaa" * nc and status[0] == 12345
        assert bytes(rs) == rng0

    over = R_.to_bytes(32, "little")                                       # the limbs of r itself: not reduced
    for rng in (False, True):
        for k in range(sp.NVEC[kind]):                                     # an unreduced scalar in each scalar input
            vecs = list(c["vecs"])
            vecs[k] = vecs[k][:FR * 3] + over
            refused(cpx.CPX_ERR_ARG, it=dict(c, vecs=tuple(vecs)), rng=rng)
        if kind == IPA:
            refused(cpx.CPX_ERR_ARG, it=dict(c, z=over), rng=rng)
        w = subarg_lib.words(c["state_in"])
        refused(cpx.CPX_ERR_ARG, state=subarg_lib.state_bytes(w[:25] + [strobe_ref.RATE, w[26]]), rng=rng)      # pos = 166
        for bad_n in (0, 3):
            refused(cpx.CPX_ERR_NOT_POW2, n=bad_n, rng=rng)
        if kind == IPA:
            refused(cpx.CPX_ERR_ARG, n=1, rng=rng)
        refused(cpx.CPX_ERR_ARG, count=(16384 if kind == IPA else 10922) + 1, rng=rng)                          # one item over the task limit: before anything is read
        per_item = 2 * 4096 + 2 if kind == IPA else 3 * 4096
        refused(cpx.CPX_ERR_ARG, count=(1 << 24) // per_item + 1, n=4096, rng=rng)                              # ... and over the point limit
        nin = len(args_of(c, d))
        for hole in list(range(nin)) + [nin, nin + 1, nin + 3]:            # every input, the states, the proofs, the status
            refused(cpx.CPX_ERR_ARG, null=hole, rng=rng)
    refused(cpx.CPX_ERR_ARG, draws=d[:FR] + over + d[2 * FR:])             # an unreduced draw
    st = (ctypes.c_uint8 * ST).from_buffer_copy(c["state_in"])
    assert fns[0](ctx._h, 0, n, *([None] * nin), st, None, None, None) == cpx.CPX_OK       # count = 0: a no-op
    assert bytes(st) == c["state_in"]
    pts, stmt, z, vecs, states = inputs(kind, [c])
    for kw in (dict(), dict(rand=d, rngs=[])):                             # neither, both
        with pytest.raises(ValueError):
            if kind == IPA:
                ctx.ipa_prove(n, *pts, *stmt, z, *vecs, states, **kw)
            else:
                ctx.same_msm_prove(n, *pts, *stmt, *vecs, states, **kw)
    # the challenges may be NULL, and the context still proves a good item
    st, proof, status = (ctypes.c_uint8 * ST).from_buffer_copy(c["state_in"]), fill(pb), (ctypes.c_int * 1)(12345)
    assert fns[0](ctx._h, 1, n, *args_of(c, d), st, proof, None, status) == cpx.CPX_OK
    w = oracle(c, d)
    assert status[0] == cpx.CPX_OK and bytes(st) == w["state"] and bytes(proof) == w["proof"]


def test_loaded_batch_is_left_alone(orc):
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
        for kind in (IPA, SMSM):
            items = [sp.sp_inputs(kind, 31 + kind, 8)] * 2
            check(c, orc, kind, 8, items, [sp.seeded_draws(orc, kind, 31 + kind, 8)] * 2)
        assert c.batch == 2
        assert c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2) == before
        assert c.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    finally:
        c.close()
