"""GPU parity of the log-round loops as one call: Context.ipa_rounds -> cpx_ipa_rounds, Context.same_msm_rounds -> cpx_same_msm_rounds.
Bytes are compared item by item with tests/subarg_lib.py: the oracle's own ipa_new / samemsm_new on seeded inputs (`case`), and where the
test chooses the entry values — zero halves, identity bases, entry states that move the rate position, a challenge that retries — the
Python restatement of the loop (`model_loop`), which tests/test_loop_rounds_cpu.py pins against the oracle's provers.  The library under
test is never the source of an expected value.

One case of the issue cannot exist: the 64 PRF bytes of a challenge never lie across byte 166 of the rate, because the PRF operation
carries the C flag and STROBE runs the permutation before it whenever pos != 0 — the bytes are always squeezed from position 0.  The third
entry state therefore puts the two header bytes of the challenge's operations across the boundary instead (a header at position 165)."""
import ctypes

import pytest

from tests import strobe_ref, subarg_lib
from tests.subarg_lib import IPA, SMSM, TERMS, IDENTITY48, R_

pytestmark = pytest.mark.gpu

FR, AFF, ST = 32, 96, 216
KINDS = pytest.mark.parametrize("kind", [IPA, SMSM], ids=["ipa", "same_msm"])
KEEP = 64 << 20
SCRATCH_BUFFERS = 35                       # include/cpx.h: 23 of the tier-0 set, 12 of the shuffle set


@pytest.fixture(scope="module")
def ctx():
    import curdleproofs_amd as cpx
    c = cpx.Context(0)                      # no CRS, nothing loaded: the loops need neither
    yield c
    assert c.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    c.close()


_cases = {}


def case(kind, seed, n, pad=0, filler=b""):
    key = (kind, seed, n, pad, filler)
    if key not in _cases:
        _cases[key] = subarg_lib.case(kind, seed, n, pad, filler)
    return _cases[key]


def item(c, **over):
    d = dict(bases=c["bases"], vecs=c["vecs"], state=c["state_in"])
    d.update(over)
    return d


def run(ctx, kind, n, items, affine=False):
    """one library call over the items; the outputs cut per item"""
    cat = lambda f: b"".join(f(i) for i in items)
    bases = [cat(lambda i, k=k: i["bases"][k]) for k in range(3)]
    vecs = [cat(lambda i, k=k: i["vecs"][k]) for k in range(len(items[0]["vecs"]))]
    states = cat(lambda i: i["state"])
    out = ctx.ipa_rounds(n, *bases, *vecs, states, affine=affine) if kind == IPA else ctx.same_msm_rounds(n, *bases, *vecs, states, affine=affine)
    L, t, nv, cnt = max(n.bit_length() - 1, 0), TERMS[kind], len(vecs), len(items)
    cut = lambda b, each: [b[each * i:each * (i + 1)] for i in range(cnt)]
    res = [dict(rounds=r, finals=f, gammas=g, state=s) for r, f, g, s in
           zip(cut(out["compressed"], L * t * 48), cut(out["finals"], nv * FR), cut(out["gammas"], L * FR), cut(out["states"], ST))]
    if affine:
        for r, a in zip(res, cut(out["affine"], L * t * AFF)):
            r["affine"] = a
    return res


def same(got, want, what=""):
    for key in ("rounds", "finals", "state"):
        assert got[key] == want[key], "%s %s" % (what, key)
    if "gammas" in want:
        assert got["gammas"] == want["gammas"], "%s gammas" % what


def oracle_of(c):
    return dict(rounds=c["rounds"], finals=c["finals"], state=c["state_out"])


# ---- against the oracle's own provers ----
@pytest.mark.parametrize("n", [2, 4, 8, 32])
@KINDS
def test_three_distinct_items_match_the_oracle(ctx, orc, kind, n):
    cs = [case(kind, 100 * n + 10 * kind + i, n, filler=bytes(range(i * 7))) for i in range(3)]
    got = run(ctx, kind, n, [item(c) for c in cs], affine=True)
    for i, (g, c) in enumerate(zip(got, cs)):
        same(g, oracle_of(c), "item %d" % i)
        assert orc.g1_compress(g["affine"]) == g["rounds"]                              # the affine output is the same points
        m = subarg_lib.model_loop(orc, kind, n, c["bases"], c["vecs"], c["state_in"])
        same(g, m, "item %d (model)" % i)                                               # ... and the challenges are the model's


@KINDS
def test_n_1_runs_no_round(ctx, orc, kind):
    rng = orc.rng(77 + kind)
    items = [dict(bases=tuple(rng.g1_affine(1) for _ in range(3)), vecs=tuple(rng.fr(1) for _ in range(2 if kind == IPA else 1)),
                  state=subarg_lib.entry_state(bytes(i))) for i in range(3)]
    for g, it in zip(run(ctx, kind, 1, items), items):
        assert g["finals"] == b"".join(it["vecs"]) and g["state"] == it["state"] and g["rounds"] == b"" and g["gammas"] == b""


def launches(ctx):
    return {k: v["launches"] for k, v in ctx.stats().items() if v["launches"]}


# Every kernel's launches in one call, as the library of the commit before the engine's sub-argument stack was split into layers made
# them: recorded by running this test's code with CPX_LIB pointing at that build.  n = 8 at counts 1 and 5; "small": IPA n = 2, SameMSM n = 1
_ROUNDS = lambda L: {"k_finalize": L, "k_loop_step": L, "k_msm_tail": L, "k_msm_tblw<2, true>": L, "k_reduce_sets": L}
LAUNCHES = {
    IPA: {1: _ROUNDS(3), 5: _ROUNDS(3), "small": _ROUNDS(1)},
    SMSM: {1: _ROUNDS(3), 5: _ROUNDS(3), "small": {}},
}


@KINDS
def test_count_1_equals_count_5_and_the_launches_depend_on_L_only(orc, kind):
    import curdleproofs_amd as cpx
    n, L = 8, 3
    c = case(kind, 31 + kind, n)
    names = ("k_msm_tblw<2, true>", "k_reduce_sets", "k_msm_tail", "k_finalize", "k_loop_step")
    ctx = cpx.Context(0)
    try:
        ctx.set_profiling(True)
        seen, table = {}, {}
        for count in (1, 5):
            ctx.reset_stats()
            got = run(ctx, kind, n, [item(c)] * count)
            for g in got:
                same(g, oracle_of(c), "count %d" % count)
            seen[count] = {k: ctx.stat(k)["launches"] for k in names}
            table[count] = launches(ctx)
            assert ctx.stat("k_loop_step")["units"] == L * count
        assert seen[1] == seen[5] == {k: L for k in names}
        ctx.reset_stats()
        if kind == IPA:                                                          # the single round of n = 2
            small = case(kind, 33, 2)
            same(run(ctx, kind, 2, [item(small)])[0], oracle_of(small), "n = 2")
        else:                                                                    # n = 1: no round, nothing launched
            rng = orc.rng(78)
            run(ctx, kind, 1, [dict(bases=tuple(rng.g1_affine(1) for _ in range(3)), vecs=(rng.fr(1),), state=subarg_lib.entry_state(b""))])
        table["small"] = launches(ctx)
        print("LAUNCHES", kind, table)
        assert table == LAUNCHES[kind]
        assert ctx.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    finally:
        ctx.close()


def test_ipa_at_1024_takes_more_than_one_slice(ctx):
    """4 tasks of 512 (+ 1) points: 64 waves leave the GPU almost empty and half of 513 points is still 256, the smallest shape for which
    the slice rule (tier0_plan.hpp tbw_slices_rule) gives more than one wave per window"""
    c = case(IPA, 1024, 1024)
    same(run(ctx, IPA, 1024, [item(c)])[0], oracle_of(c))


# ---- entry values chosen by the test, against the model ----
def _one_round(orc, kind):
    c = case(kind, 5 + kind, 2)
    return c, subarg_lib.model_loop(orc, kind, 2, c["bases"], c["vecs"], c["state_in"])["rounds"]


@KINDS
def test_entry_states_that_put_a_point_a_label_and_a_header_across_the_rate_boundary(ctx, orc, kind):
    c, enc = _one_round(orc, kind)
    found = {}
    for f in range(1, 2 * strobe_ref.RATE):
        st = subarg_lib.entry_state(bytes(f))
        t, _, _ = subarg_lib.round_transcript(kind, st, enc)
        if "point" not in found and any(n == 48 for _, n in strobe_ref.splits(t.trace, "data")):
            found["point"] = st
        elif "label" not in found and strobe_ref.splits(t.trace, "label"):
            found["label"] = st
        elif "header" not in found and ("header", strobe_ref.RATE - 1) in t.trace:
            found["header"] = st
        if len(found) == 3:
            break
    assert sorted(found) == ["header", "label", "point"]
    items = [item(c, state=found[k]) for k in ("point", "label", "header")]
    for g, it in zip(run(ctx, kind, 2, items), items):
        same(g, subarg_lib.model_loop(orc, kind, 2, it["bases"], it["vecs"], it["state"]))


@KINDS
def test_a_challenge_that_retries(ctx, orc, kind):
    """about 9.4 % of the draws are refused: entry states are searched in the model until one round's challenge takes two attempts"""
    c, enc = _one_round(orc, kind)
    for f in range(300):
        st = subarg_lib.entry_state(b"retry" + f.to_bytes(2, "little"))
        if subarg_lib.round_transcript(kind, st, enc)[2] > 1:
            break
    items = [item(c), item(c, state=st)]
    want = [subarg_lib.model_loop(orc, kind, 2, i["bases"], i["vecs"], i["state"]) for i in items]
    assert want[1]["attempts"][0] > 1 and ("attempt", False) in want[1]["trace"]
    for g, w in zip(run(ctx, kind, 2, items), want):
        same(g, w)


@KINDS
def test_identity_bases(ctx, kind):
    """the reference pads T and U with the identity beside the two blinder bases (curdleproofs.rs:141-155); G' likewise here"""
    c = case(kind, 61 + kind, 8, pad=4)
    assert c["bases"][1][-AFF:] == bytes(AFF) if kind == IPA else c["bases"][1][4 * AFF:6 * AFF] == bytes(2 * AFF)
    same(run(ctx, kind, 8, [item(c)])[0], oracle_of(c))


def test_vec_x_zero_on_one_half_hashes_three_identities(ctx, orc):
    c = case(SMSM, 71, 4)
    x = c["vecs"][0][:2 * FR] + bytes(2 * FR)                  # x_R = 0: R_A, R_T, R_U of the first round are the identity
    it = item(c, vecs=(x,))
    want = subarg_lib.model_loop(orc, SMSM, 4, it["bases"], it["vecs"], it["state"])
    assert want["rounds"][3 * 48:6 * 48] == IDENTITY48 * 3 and IDENTITY48 not in (want["rounds"][:48], want["rounds"][6 * 48:7 * 48])
    same(run(ctx, SMSM, 4, [it])[0], want)


def test_zero_inner_products(ctx, orc):
    c = case(IPA, 72, 4)
    a, b = subarg_lib.to_ints(orc, c["vecs"][0]), subarg_lib.to_ints(orc, c["vecs"][1])
    cv = subarg_lib.to_wire(orc, [a[0], 0, 0, a[3]])           # <c_L, d_R> = <c_R, d_L> = 0 with no vector zero
    dv = subarg_lib.to_wire(orc, [b[0], 0, 0, b[3]])
    zero = item(c, vecs=(cv, bytes(4 * FR)))                   # ... and with d = 0: L_D and R_D are the identity as well
    items = [item(c, vecs=(cv, dv)), zero]
    want = [subarg_lib.model_loop(orc, IPA, 4, i["bases"], i["vecs"], i["state"]) for i in items]
    assert want[1]["rounds"][48:96] == IDENTITY48 and want[1]["rounds"][3 * 48:4 * 48] == IDENTITY48
    for g, w in zip(run(ctx, IPA, 4, items), want):
        same(g, w)


# ---- stand-alone proofs end to end ----
@KINDS
def test_standalone_proof_bytes_at_n_32(ctx, orc, kind):
    """the steps before the loop from the shim, then ONE library call: the oracle's serialised InnerProductProof / SameMultiscalarProof"""
    n, L, t = 32, 5, TERMS[kind]
    c = case(kind, 320 + kind, n, pad=2 if kind == SMSM else 0)
    g = run(ctx, kind, n, [item(c)])[0]
    pts = [[g["rounds"][(j * t + q) * 48:(j * t + q + 1) * 48] for j in range(L)] for q in range(t)]
    order = (0, 2, 1, 3) if kind == IPA else range(6)          # inner_product_argument.rs:328-338, same_multiscalar_argument.rs:263-275
    assert c["pre"] + b"".join(b"".join(pts[q]) for q in order) + orc.fr_to_canonical_bytes(g["finals"]) == c["proof"]
    assert g["state"] == c["state_out"]


# ---- conventions ----
def _raw(ctx, kind, count, n, it, outs):
    args = list(it["bases"]) + list(it["vecs"])
    fn = ctx._L.cpx_ipa_rounds if kind == IPA else ctx._L.cpx_same_msm_rounds
    return fn(ctx._h, count, n, *args, *outs)


@KINDS
def test_either_points_output_and_the_gammas_may_be_null(ctx, kind):
    import curdleproofs_amd as cpx
    n, L, t = 4, 2, TERMS[kind]
    c = case(kind, 41 + kind, n)
    nv = len(c["vecs"])
    full = run(ctx, kind, n, [item(c)], affine=True)[0]
    fill = lambda size: (ctypes.c_uint8 * size)(*([0xaa] * size))
    for keep in ((1, 0, 1), (0, 1, 0), (0, 0, 0)):
        st = (ctypes.c_uint8 * ST).from_buffer_copy(c["state_in"])
        comp, aff, fin, gam = fill(L * t * 48), fill(L * t * AFF), fill(nv * FR), fill(L * FR)
        outs = [st, comp if keep[0] else None, aff if keep[1] else None, fin, gam if keep[2] else None]
        assert _raw(ctx, kind, 1, n, item(c), outs) == cpx.CPX_OK
        assert bytes(st) == c["state_out"] and bytes(fin) == c["finals"]
        assert bytes(comp) == (c["rounds"] if keep[0] else b"\xaa" * (L * t * 48))
        assert bytes(aff) == (full["affine"] if keep[1] else b"\xaa" * (L * t * AFF))
        assert bytes(gam) == (full["gammas"] if keep[2] else b"\xaa" * (L * FR))


@KINDS
def test_refusals_write_nothing(ctx, kind):
    import curdleproofs_amd as cpx
    n, L, t = 4, 2, TERMS[kind]
    c = case(kind, 41 + kind, n)
    nv = len(c["vecs"])
    fill = lambda size: (ctypes.c_uint8 * size)(*([0xaa] * size))
    sizes = (L * t * 48, L * t * AFF, nv * FR, L * FR)

    def refused(code, count=1, n=n, it=None, state=None, null=None):
        st = (ctypes.c_uint8 * ST).from_buffer_copy(state or c["state_in"])
        bufs = [fill(s) for s in sizes]
        outs = [st] + bufs
        it = it or item(c)
        args = list(it["bases"]) + list(it["vecs"])
        if null is not None:
            if null < len(args):
                args[null] = None
            else:
                outs[null - len(args)] = None
        fn = ctx._L.cpx_ipa_rounds if kind == IPA else ctx._L.cpx_same_msm_rounds
        assert fn(ctx._h, count, n, *args, *outs) == code
        assert bytes(st) == (state or c["state_in"]) and all(bytes(b) == b"\xaa" * s for b, s in zip(bufs, sizes))

    over = R_.to_bytes(32, "little")                                       # the limbs of r itself: not reduced
    for v in range(nv):
        vecs = list(c["vecs"])
        vecs[v] = vecs[v][:FR * 3] + over
        refused(cpx.CPX_ERR_ARG, it=item(c, vecs=tuple(vecs)))
    w = subarg_lib.words(c["state_in"])
    refused(cpx.CPX_ERR_ARG, state=subarg_lib.state_bytes(w[:25] + [strobe_ref.RATE, w[26]]))
    refused(cpx.CPX_ERR_ARG, state=subarg_lib.state_bytes(w[:25] + [w[25], strobe_ref.RATE + 1]))
    for bad_n in (0, 3, 6):
        refused(cpx.CPX_ERR_NOT_POW2, n=bad_n)
    refused(cpx.CPX_ERR_ARG, count=(16384 if kind == IPA else 10922) + 1)  # one item more than a round's 2^16 tasks hold: before anything is read
    refused(cpx.CPX_ERR_ARG, count=5000, n=1 << 12)                         # ... and than its 2^24 points
    nin = 3 + nv
    for hole in list(range(nin)) + [nin, nin + 3]:                          # every input, the states, the finals
        refused(cpx.CPX_ERR_ARG, null=hole)
    st = (ctypes.c_uint8 * ST).from_buffer_copy(c["state_in"])
    assert _raw(ctx, kind, 0, n, item(c), [st, None, None, None, None]) == cpx.CPX_OK      # count = 0: a no-op
    assert bytes(st) == c["state_in"]


def test_loaded_batch_is_left_alone(orc):
    import curdleproofs_amd as cpx
    ell = 28
    crs = orc.generate_crs_points(ell)
    inst = orc.make_instance(ell, 0, crs)
    cs = {kind: case(kind, 31 + kind, 8) for kind in (IPA, SMSM)}
    c = cpx.Context(0)
    try:
        c.set_crs(ell, crs)
        c.load_batch(*(inst[k] * 2 for k in ("vec_R", "vec_S", "vec_T", "vec_U", "M")))
        before = c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2)
        assert c.batch == 2 and before == [cpx.CPX_OK] * 2
        for kind in (IPA, SMSM):
            same(run(c, kind, 8, [item(cs[kind])] * 2)[1], oracle_of(cs[kind]))
        assert c.batch == 2
        assert c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2) == before
        assert c.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    finally:
        c.close()
