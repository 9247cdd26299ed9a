"""GPU parity of the stand-alone sub-argument verifiers: Context.ipa_verify -> cpx_ipa_verify, Context.same_msm_verify ->
cpx_same_msm_verify.  Verdicts, states and challenges are compared item by item with tests/subarg_verify_lib.py: the oracle's own
ipa_verify / samemsm_verify on the very inputs the library gets (a fresh transcript, a fresh accumulator, the same draws).  The library
under test is never the source of an expected value; tests/test_subarg_verify_cpu.py shows on the CPU that every change made here is one
the flattened check notices.

The retrying challenge is covered by tests/test_gpu_transcript.py on the same WaveStrobe and is not repeated."""
import ctypes

import pytest

from tests import decoding_ref, strobe_ref, subarg_lib, subarg_verify_lib as sv
from tests.subarg_lib import IPA, SMSM, IDENTITY48, R_

pytestmark = pytest.mark.gpu

FR, AFF, JAC, ST = 32, 96, 144, 216
KINDS = pytest.mark.parametrize("kind", [IPA, SMSM], ids=["ipa", "same_msm"])
KEEP = 64 << 20
SCRATCH_BUFFERS = 35                       # include/cpx.h: 23 of the tier-0 set, 12 of the shuffle set


@pytest.fixture(scope="module")
def ctx():
    import curdleproofs_amd as cpx
    c = cpx.Context(0)                      # no CRS, nothing loaded: the verifiers need neither
    yield c
    assert c.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    c.close()


def inputs(kind, items):
    cat = lambda f: b"".join(f(i) for i in items)
    pts = [cat(lambda i, k=k: i["bases"][k]) for k in range(sv.FAMILIES[kind])]
    stmt = [cat(lambda i, k=k: i["stmt"][k]) for k in range(3)]
    return pts, stmt, cat(lambda i: i["z"]), cat(lambda i: i["vec_u"]), cat(lambda i: i["proof"]), cat(lambda i: i["state_in"])


def run(ctx, kind, n, items, rand):
    """one library call over the items; per item dict(verdict, state, challenges)"""
    from curdleproofs_amd.whisk import SerializationError
    pts, stmt, z, u, proofs, states = inputs(kind, items)
    if kind == IPA:
        out = ctx.ipa_verify(n, pts[0], *stmt, z, u, proofs, rand, states, challenges=True)
    else:
        out = ctx.same_msm_verify(n, *pts, *stmt, proofs, rand, states, challenges=True)
    code = lambda v: sv.OK if v is True else sv.ERR_VERIFY if v is False else sv.ERR_DESERIALIZE if isinstance(v, SerializationError) else None
    nc = sv.n_challenges(kind, sv.log2(n)) * FR
    return [dict(verdict=code(v), state=out["states"][ST * i:ST * (i + 1)], challenges=out["challenges"][nc * i:nc * (i + 1)])
            for i, v in enumerate(out["verdicts"])]


def rand_of(rand, kind, i):
    k = sv.CHECKS[kind] * FR
    return rand[k * i:k * (i + 1)]


_oracle = {}


def oracle(c, rand):
    key = (c["kind"], c["n"], c["filler"], c["bases"], c["stmt"], c["z"], c["vec_u"], c["proof"], rand)
    if key not in _oracle:
        _oracle[key] = sv.verify(c, rand)
    return _oracle[key]


def check(ctx, orc, kind, n, items, seed, expect=None, one_draw=False):
    """the call against the oracle, item by item; expect: the verdicts the test means to provoke (the oracle must give them too).
    one_draw: every item gets the same random factors (equal items then cost the oracle one run)"""
    rand = sv.factors(orc, seed, kind) * len(items) if one_draw else sv.factors(orc, seed, kind, len(items))
    got = run(ctx, kind, n, items, rand)
    want = [oracle(c, rand_of(rand, kind, i)) for i, c in enumerate(items)]
    for i, (g, w) in enumerate(zip(got, want)):
        for key in ("verdict", "state", "challenges"):
            assert g[key] == w[key], "item %d: %s" % (i, key)
    if expect is not None:
        assert [w["verdict"] for w in want] == list(expect)
    return got


def three(kind, n, base):
    return [sv.make(kind, base + i, n, filler=bytes(range(7 * i))) for i in range(3)]


# ---- accepted proofs ----
@pytest.mark.parametrize("n", [1, 2, 4, 8])
@KINDS
def test_three_distinct_valid_items(ctx, orc, kind, n):
    check(ctx, orc, kind, n, three(kind, n, 1000 * n + 100 * kind), 50 + n, expect=[sv.OK] * 3)


@pytest.mark.parametrize("n", [64, 256])     # a row one wave wide; more elements than the work-group has threads
@KINDS
def test_rows_wider_than_a_wave_and_than_the_group(ctx, orc, kind, n):
    items = [sv.make(kind, 3 * n + kind, n), sv.make(kind, 3 * n + kind + 7, n, filler=bytes(100))]
    check(ctx, orc, kind, n, items, 60 + n, expect=[sv.OK] * 2)


# Every kernel's launches in one call, as the library of the commit before the engine's sub-argument stack was split into layers made
# them: recorded by running this test's code with CPX_LIB pointing at that build.  n = 8 at counts 1 and 5; "small": IPA n = 2, SameMSM n = 1
_IPA_ANY = {"k_decompress": 1, "k_finalize": 1, "k_msm_tail": 1, "k_msm_tblw<2, true>": 1, "k_reduce_sets": 1, "k_subarg_scalars": 1}
_SMSM_ANY = {"k_compress": 1, "k_decompress": 1, "k_finalize": 1, "k_msm_tail": 1, "k_msm_tblw<2, true>": 1, "k_reduce_sets": 1, "k_subarg_scalars": 1}
LAUNCHES = {
    IPA: {1: _IPA_ANY, 5: _IPA_ANY, "small": _IPA_ANY},
    SMSM: {1: _SMSM_ANY, 5: _SMSM_ANY, "small": _SMSM_ANY},
}


@KINDS
def test_count_1_equals_count_5_and_the_launches_depend_on_L_only(orc, kind):
    import curdleproofs_amd as cpx
    n = 8
    c = sv.make(kind, 31 + kind, n)
    names = ["k_decompress", "k_finalize", "k_subarg_scalars", "k_msm_tblw<2, true>", "k_reduce_sets", "k_msm_tail"] + (["k_compress"] if kind == SMSM else [])
    ctx = cpx.Context(0)
    try:
        ctx.set_profiling(True)
        seen, table = {}, {}
        for count in (1, 5):
            ctx.reset_stats()
            check(ctx, orc, kind, n, [c] * count, 70 + count, expect=[sv.OK] * count)
            seen[count] = {k: ctx.stat(k)["launches"] for k in names}
            table[count] = {k: v["launches"] for k, v in ctx.stats().items() if v["launches"]}
            assert ctx.stat("k_subarg_scalars")["units"] == count and "k_subarg_scalars" in ctx.stats()
        assert seen[1] == seen[5] == {k: 1 for k in names}
        m = 2 if kind == IPA else 1                                            # one round's points; n = 1: none
        ctx.reset_stats()
        check(ctx, orc, kind, m, [sv.make(kind, 41 + kind, m)], 76, expect=[sv.OK])
        table["small"] = {k: v["launches"] for k, v in ctx.stats().items() if v["launches"]}
        print("LAUNCHES", kind, table)
        assert table == LAUNCHES[kind]
        assert ctx.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    finally:
        ctx.close()


@KINDS
def test_70_items_in_one_call(ctx, orc, kind):
    """more tasks than one slice of the MSM waves takes; one item among them is wrong"""
    n = 8
    cs = [sv.make(kind, 400 + kind + i, n, filler=bytes(i)) for i in range(5)]
    items = [cs[i % 5] for i in range(70)]
    items[37] = list(sv.mutations(orc, items[37]).values())[1]
    got = check(ctx, orc, kind, n, items, 77, expect=[sv.OK] * 37 + [sv.ERR_VERIFY] + [sv.OK] * 32, one_draw=True)
    assert got[2]["state"] == got[7]["state"] and got[2]["challenges"] == got[7]["challenges"]


# ---- one item wrong among valid neighbours ----
_valid = {}


def neighbours(ctx, orc, kind, n):
    """(items, rand seed, the all-valid call's results), once per kind"""
    if (kind, n) not in _valid:
        items = three(kind, n, 5000 + 100 * kind)
        _valid[(kind, n)] = (items, check(ctx, orc, kind, n, items, 91, expect=[sv.OK] * 3))
    return _valid[(kind, n)]


def one_wrong(ctx, orc, kind, n, changed, verdict):
    items, valid = neighbours(ctx, orc, kind, n)
    got = check(ctx, orc, kind, n, [items[0], changed, items[2]], 91, expect=[sv.OK, verdict, sv.OK])
    assert got[0] == valid[0] and got[2] == valid[2]                       # the neighbours as in the all-valid call
    return got[1]


MUTATIONS = {IPA: ("z + 1", "c_final + 1", "one vec_u entry", "L and R swapped", "another L_D"),
             SMSM: ("x_final + 1", "L and R swapped", "B_t = B_u", "a base of T")}


@pytest.mark.parametrize("kind,name", [(k, m) for k in (IPA, SMSM) for m in MUTATIONS[k]], ids=lambda v: v if isinstance(v, str) else ("ipa", "same_msm")[v])
def test_one_item_rejected(ctx, orc, kind, name):
    n = 8
    items, _ = neighbours(ctx, orc, kind, n)
    one_wrong(ctx, orc, kind, n, sv.mutations(orc, items[1])[name], sv.ERR_VERIFY)


def _defects(orc, kind, L, proof):
    """name -> the proof with one undecodable part"""
    mid = sv.slot(kind, L, "R_D" if kind == IPA else "L_U", 1)
    last = sv.proof_points(kind, L) - 1
    enc = lambda x: decoding_ref.encode(x, 0x80)
    orig = sv.point(proof, 0)
    return {"an x not on the curve": sv.with_point(proof, mid, enc(decoding_ref.off_curve_xs(1)[0])),
            "a point outside the subgroup": sv.with_point(proof, last, enc(decoding_ref.non_member_points(orc, 1)[0][0])),
            "a scalar equal to r": sv.with_scalar(kind, L, proof, 1 if kind == IPA else 0, R_),
            "a cleared compression flag": sv.with_point(proof, 0, bytes([orig[0] & 0x7f]) + orig[1:])}


@pytest.mark.parametrize("name", ["an x not on the curve", "a point outside the subgroup", "a scalar equal to r", "a cleared compression flag"])
@KINDS
def test_one_item_does_not_deserialise(ctx, orc, kind, name):
    n = 8
    items, _ = neighbours(ctx, orc, kind, n)
    bad = dict(items[1], proof=_defects(orc, kind, 3, items[1]["proof"])[name])
    got = one_wrong(ctx, orc, kind, n, bad, sv.ERR_DESERIALIZE)
    nc = sv.n_challenges(kind, 3) * FR
    assert got["state"] == items[1]["state_in"] and got["challenges"] == bytes(nc)   # the reference never reaches `verify`


# ---- the identity and the rate position ----
@KINDS
def test_identity_encodings_are_legal(ctx, orc, kind):
    """among the round points and as a B point: the verdict is the oracle's (a rejection: the proof was not made that way); the one
    IPA proof of n = 1 has B_c = B_d = O and is accepted (test_three_distinct_valid_items)"""
    n, L = 4, 2
    c = sv.make(kind, 640 + kind, n)
    round_pt = dict(c, proof=sv.with_point(c["proof"], sv.slot(kind, L, "R_D" if kind == IPA else "R_U", 1), IDENTITY48))
    b_pt = dict(c, proof=sv.with_point(c["proof"], sv.slot(kind, L, "B_d" if kind == IPA else "B_u"), IDENTITY48))
    check(ctx, orc, kind, n, [round_pt, c, b_pt], 64, expect=[sv.ERR_VERIFY, sv.OK, sv.ERR_VERIFY])
    if kind == IPA:
        one = sv.make(IPA, 641, 1)
        assert one["proof"][:96] == IDENTITY48 * 2
        check(ctx, orc, IPA, 1, [one], 65, expect=[sv.OK])


@KINDS
def test_entry_states_that_put_a_point_a_label_and_a_header_across_the_rate_boundary(ctx, orc, kind):
    """filler lengths are searched in the Python model of the transcript (pinned to the oracle on the CPU) until `verify` has had a
    48-byte encoding, a label and an operation header cut by byte 166 of the rate"""
    n = 2
    found = {}
    for f in range(1, 2 * strobe_ref.RATE):
        c = sv.make(kind, 680 + kind, n, filler=bytes(f))
        t, _ = sv.model_transcript(orc, c)
        if "point" not in found and any(size == 48 for _, size in strobe_ref.splits(t.trace, "data")):
            found["point"] = c
        elif "label" not in found and strobe_ref.splits(t.trace, "label"):
            found["label"] = c
        elif "header" not in found and ("header", strobe_ref.RATE - 1) in t.trace:
            found["header"] = c
        if len(found) == 3:
            break
    assert sorted(found) == ["header", "label", "point"]
    check(ctx, orc, kind, n, [found[k] for k in ("point", "label", "header")], 68, expect=[sv.OK] * 3)


# ---- round trip on the device ----
@KINDS
def test_a_proof_from_the_rounds_call_is_accepted(ctx, orc, kind):
    """the steps before the loop from the shim, the loop from Context.ipa_rounds / same_msm_rounds, the bytes assembled as `serialize`
    writes them, then the new call"""
    n, L = 16, 4
    terms = subarg_lib.TERMS[kind]
    c = sv.make(kind, 720 + kind, n, filler=b"round trip")
    e = sv.loop_entry(kind, 720 + kind, n, filler=b"round trip")
    out = ctx.ipa_rounds(n, *e["bases"], *e["vecs"], e["state"]) if kind == IPA else ctx.same_msm_rounds(n, *e["bases"], *e["vecs"], e["state"])
    rounds = out["compressed"]
    pts = [[rounds[(j * terms + q) * 48:(j * terms + q + 1) * 48] for j in range(L)] for q in range(terms)]
    order = (0, 2, 1, 3) if kind == IPA else range(6)          # inner_product_argument.rs:328-338, same_multiscalar_argument.rs:263-275
    proof = e["pre"] + b"".join(b"".join(pts[q]) for q in order) + orc.fr_to_canonical_bytes(out["finals"])
    assert len(proof) == sv.proof_bytes(kind, L)
    got = check(ctx, orc, kind, n, [dict(c, proof=proof)], 72, expect=[sv.OK])
    assert got[0]["state"] == out["states"]                    # prover and verifier leave the same transcript


# ---- refusals ----
@KINDS
def test_refusals_write_nothing(ctx, orc, kind):
    import curdleproofs_amd as cpx
    n, L = 4, 2
    c = sv.make(kind, 41 + kind, n)
    rand = sv.factors(orc, 43, kind)
    nc = sv.n_challenges(kind, L) * FR
    fill = lambda size: (ctypes.c_uint8 * size)(*([0xaa] * size))
    fn = ctx._L.cpx_ipa_verify if kind == IPA else ctx._L.cpx_same_msm_verify

    def args_of(it, rand):
        pts, stmt, z, u, proofs, _ = inputs(kind, [it])
        return ([pts[0]] + stmt + [z, u] if kind == IPA else pts + stmt) + [proofs, rand]

    def refused(code, count=1, n=n, it=None, rand=rand, state=None, null=None):
        st = (ctypes.c_uint8 * ST).from_buffer_copy(state or c["state_in"])
        chal, ver = fill(nc), (ctypes.c_int * 1)(12345)
        args = args_of(it or c, rand)
        outs = [st, chal, ver]
        if null is not None:
            if null < len(args):
                args[null] = None
            else:
                outs[null - len(args)] = None
        assert fn(ctx._h, count, n, *args, *outs) == code
        assert bytes(st) == (state or c["state_in"]) and bytes(chal) == b"\xaa" * nc and ver[0] == 12345

    over = R_.to_bytes(32, "little")                                       # the limbs of r itself: not reduced
    for k in range(sv.CHECKS[kind]):
        refused(cpx.CPX_ERR_ARG, rand=rand[:FR * k] + bytes(FR) + rand[FR * (k + 1):])     # a zero factor
        refused(cpx.CPX_ERR_ARG, rand=rand[:FR * k] + over + rand[FR * (k + 1):])          # a factor >= r
    if kind == IPA:
        refused(cpx.CPX_ERR_ARG, it=dict(c, vec_u=c["vec_u"][:FR * 3] + over))
        refused(cpx.CPX_ERR_ARG, it=dict(c, z=over))
    w = subarg_lib.words(c["state_in"])
    refused(cpx.CPX_ERR_ARG, state=subarg_lib.state_bytes(w[:25] + [strobe_ref.RATE, w[26]]))             # pos > 165
    refused(cpx.CPX_ERR_ARG, state=subarg_lib.state_bytes(w[:25] + [w[25], strobe_ref.RATE + 1]))
    for bad_n in (0, 3):
        refused(cpx.CPX_ERR_NOT_POW2, n=bad_n)
    refused(cpx.CPX_ERR_ARG, count=(1 << 16) + 1)                          # one item more than 2^16 tasks: before anything is read
    refused(cpx.CPX_ERR_ARG, count=5000, n=1 << 12)                        # ... and count * points over 2^24
    nin = len(args_of(c, rand))
    for hole in list(range(nin)) + [nin, nin + 2]:                         # every input, the states, the verdicts
        refused(cpx.CPX_ERR_ARG, null=hole)
    st = (ctypes.c_uint8 * ST).from_buffer_copy(c["state_in"])
    assert fn(ctx._h, 0, n, *([None] * nin), st, None, None) == cpx.CPX_OK                 # count = 0: a no-op
    assert bytes(st) == c["state_in"]
    st, ver = (ctypes.c_uint8 * ST).from_buffer_copy(c["state_in"]), (ctypes.c_int * 1)(12345)
    assert fn(ctx._h, 1, n, *args_of(c, rand), st, None, ver) == cpx.CPX_OK                # the challenges may be NULL
    assert ver[0] == cpx.CPX_OK and bytes(st) == sv.verify(c, rand)["state"]


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
            check(c, orc, kind, 8, [sv.make(kind, 31 + kind, 8)] * 2, 99, expect=[sv.OK] * 2)
        assert c.batch == 2
        assert c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2) == before
        assert c.get_option("tier0_scratch_bytes") <= SCRATCH_BUFFERS * KEEP
    finally:
        c.close()
