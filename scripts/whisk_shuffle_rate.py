"""Rates of the batched Whisk shuffle-proof calls against a loop over the single-proof calls, on one context.

    python scripts/whisk_shuffle_rate.py [--ell 124] [--counts 1,64,1024] [--runs 5] [--step-ell 252] [--step-count 1024] [--out FILE.txt]

For every count: one batched cpx_whisk_generate_shuffle_proofs / cpx_whisk_verify_shuffle_proofs call against `count` calls of
cpx_whisk_generate_shuffle_proof / cpx_whisk_is_valid_shuffle_proof on the same items (the single calls are the code this library had
before the batched ones existed).  Then the shuffle step alone (cpx_batch_shuffle, util.rs:83-106 — the column benches/perf.rs:26-49
reports) in instances per second at --step-ell.

Inputs are seeded (random.Random: reproducible, CSPRNG-free); 64 distinct tracker lists are tiled to the largest count, every item has
its own permutation, k, blinders and draws.  Timing is at the C-ABI with the buffers marshalled beforehand.  Batched calls: one warm-up
per shape, then the median of --runs timed calls.  Single-call loops: the loop of the smallest count is the warm-up of all of them; loops
of up to 64 items are timed --runs times (median), longer ones once (a loop of 1024 single calls lasts tens of seconds).  Exit status 1
if a batched result differs from the single call's or a verdict is not CPX_OK.
"""
import argparse
import ctypes
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import curdleproofs_amd as cpx   # noqa: E402
from curdleproofs_amd import crs as crsmod, params   # noqa: E402

DISTINCT = 64
SEED = "whisk_shuffle_rate"


def compress(ctx, aff):
    one = params.fp_to_wire(1)
    n = len(aff) // 96
    return ctx.normalize(b"".join(aff[96 * i:96 * (i + 1)] + one for i in range(n)), compressed=True)[1]


def make_items(ctx, ell, count, rng):
    """count items: affine vec_R / vec_S, the same as compressed pre trackers, permutation, k, blinders, prover draws, verifier factors"""
    n, d = ell + 4, min(count, DISTINCT)
    vec_r = ctx.scale(params.g1_generator_wire() * (d * ell), params.random_fr_wire(rng, d * ell))
    vec_s = ctx.scale(vec_r, params.random_fr_wire(rng, d * ell))
    cr, cs = compress(ctx, vec_r), compress(ctx, vec_s)
    pre = b"".join(cr[48 * i:48 * (i + 1)] + cs[48 * i:48 * (i + 1)] for i in range(d * ell))
    tile = lambda blob, per: b"".join(blob[per * (i % d):per * (i % d + 1)] for i in range(count))
    perm = []
    for _ in range(count):
        p = list(range(ell))
        rng.shuffle(p)
        perm += p
    return dict(vec_R=tile(vec_r, 96 * ell), vec_S=tile(vec_s, 96 * ell), pre=tile(pre, 96 * ell), perm=perm, k=params.random_fr_wire(rng, count),
                mb=params.random_fr_wire(rng, 4 * count), rand=params.random_fr_wire(rng, (3 * n + 9) * count), vrand=params.random_fr_wire(rng, 8 * count))


def timed(fn, runs, warm=True):
    if warm:
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ell", type=int, default=124)
    ap.add_argument("--counts", default="1,64,1024")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--step-ell", type=int, default=252)
    ap.add_argument("--step-count", type=int, default=1024)
    ap.add_argument("--out")
    a = ap.parse_args()
    counts = sorted(int(c) for c in a.counts.split(","))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = cpx.Context(0)
    L, h = ctx._L, ctx._h
    ell, n = a.ell, a.ell + 4
    crsmod.crs_from_seed(ctx, ell, SEED)
    rec = 48 + ctx.proof_size
    it = make_items(ctx, ell, counts[-1], random.Random(20261017))
    ok = True
    say("# whisk_shuffle_rate: ell = %d, proof record %d B, runs = %d, device_min_batch = %d, fix_bits = %d" %
        (ell, rec, a.runs, ctx.get_option("device_min_batch"), ctx.get_option("fix_bits_effective")))
    say("# count | generate: batched ms, proofs/s | single loop ms, proofs/s | ratio || verify: batched ms, proofs/s | single loop ms, proofs/s | ratio")
    first_loop = True
    for c in counts:
        pre, k, mb, rand, vrand = (cpx._in(x) for x in (it["pre"][:96 * ell * c], it["k"][:32 * c], it["mb"][:128 * c], it["rand"][:32 * (3 * n + 9) * c],
                                                        it["vrand"][:256 * c]))
        perm = (ctypes.c_uint32 * (c * ell))(*it["perm"][:c * ell])
        post, proofs = cpx._out(96 * ell * c), cpx._out(rec * c)
        st, verdict = (ctypes.c_int * c)(), (ctypes.c_int * c)()
        gen = lambda: ctx._check(L.cpx_whisk_generate_shuffle_proofs(h, c, pre, perm, k, mb, rand, post, proofs, st))
        t_gen = timed(gen, a.runs)
        ok &= all(s == cpx.CPX_OK for s in st)
        ver = lambda: ctx._check(L.cpx_whisk_verify_shuffle_proofs(h, c, pre, post, proofs, vrand, verdict))
        t_ver = timed(ver, a.runs)
        ok &= all(v == cpx.CPX_OK for v in verdict)
        pb, fb = bytes(post), bytes(proofs)
        # the single calls, one item after the other
        single = [(cpx._in(it["pre"][96 * ell * i:96 * ell * (i + 1)]), (ctypes.c_uint32 * ell)(*it["perm"][ell * i:ell * (i + 1)]), cpx._in(it["k"][32 * i:32 * (i + 1)]),
                   cpx._in(it["mb"][128 * i:128 * (i + 1)]), cpx._in(it["rand"][32 * (3 * n + 9) * i:32 * (3 * n + 9) * (i + 1)]),
                   cpx._in(it["vrand"][256 * i:256 * (i + 1)]), cpx._out(96 * ell), cpx._out(rec)) for i in range(c)]
        valid = ctypes.c_int(0)

        def single_generate():
            for p_, pm_, k_, mb_, r_, _, po_, pf_ in single:
                ctx._check(L.cpx_whisk_generate_shuffle_proof(h, p_, pm_, k_, mb_, r_, po_, pf_))

        def single_verify():
            for p_, _, _, _, _, vr_, po_, pf_ in single:
                ctx._check(L.cpx_whisk_is_valid_shuffle_proof(h, p_, po_, pf_, vr_, ctypes.byref(valid)))
                assert valid.value == 1

        loop_runs = a.runs if c <= 64 else 1
        t_sg = timed(single_generate, loop_runs, warm=first_loop)
        t_sv = timed(single_verify, loop_runs, warm=first_loop)
        first_loop = False
        ok &= all(bytes(s_[6]) == pb[96 * ell * i:96 * ell * (i + 1)] and bytes(s_[7]) == fb[rec * i:rec * (i + 1)] for i, s_ in enumerate(single))
        say("%5d | %9.2f %10.1f | %10.2f %8.1f | %7.2fx || %9.2f %10.1f | %10.2f %8.1f | %7.2fx" %
            (c, 1e3 * t_gen, c / t_gen, 1e3 * t_sg, c / t_sg, t_sg / t_gen, 1e3 * t_ver, c / t_ver, 1e3 * t_sv, c / t_sv, t_sv / t_ver))
    # the shuffle step alone
    ell, c = a.step_ell, a.step_count
    crsmod.crs_from_seed(ctx, ell, SEED)
    it = make_items(ctx, ell, c, random.Random(20261018))
    r_, s_, k, mb = (cpx._in(x) for x in (it["vec_R"], it["vec_S"], it["k"], it["mb"]))
    perm = (ctypes.c_uint32 * (c * ell))(*it["perm"])
    t_out, u_out, m_out = cpx._out(96 * ell * c), cpx._out(96 * ell * c), cpx._out(144 * c)
    t_step = timed(lambda: ctx._check(L.cpx_batch_shuffle(h, c, r_, s_, perm, k, mb, t_out, u_out, m_out)), a.runs)
    one = (cpx._in(it["vec_R"][:96 * ell]), cpx._in(it["vec_S"][:96 * ell]), (ctypes.c_uint32 * ell)(*it["perm"][:ell]), cpx._in(it["k"][:32]), cpx._in(it["mb"][:128]))
    t_one = timed(lambda: ctx._check(L.cpx_batch_shuffle(h, 1, one[0], one[1], one[2], one[3], one[4], t_out, u_out, m_out)), a.runs)
    say("# shuffle step (cpx_batch_shuffle), ell = %d: %d instances in %.2f ms = %.1f instances/s; one instance per call: %.2f ms = %.1f instances/s" %
        (ell, c, 1e3 * t_step, c / t_step, 1e3 * t_one, 1 / t_one))
    say("# all results as expected: %s" % bool(ok))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
