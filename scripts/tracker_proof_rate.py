"""Rates of the batched tracker-proof calls against a loop over the single-proof calls, on one context.

    python scripts/tracker_proof_rate.py [--counts 64,1024,16384] [--runs 5] [--single 64] [--out FILE.json]

Inputs are seeded (params.random_fr_wire with random.Random: reproducible, CSPRNG-free).  One warm-up per shape, then the median of
`--runs` timed calls at the C-ABI with the buffers marshalled beforehand, so that neither side pays Python copies.  The single-proof
loop runs cpx_whisk_is_valid_tracker_proof / cpx_whisk_generate_tracker_proof over the first `--single` items.  With profiling on, one
more call per count gives the kernel times (Context.stat).  Prints one JSON object; exit status 1 if a batched verdict is not CPX_OK
or a batched proof differs from the single call's.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import curdleproofs_amd as cpx   # noqa: E402
from curdleproofs_amd import params   # noqa: E402

KERNELS = ("k_decompress", "k_tracker_challenge", "k_tracker_relations", "k_smul", "k_compress")


def make_inputs(ctx, n, seed=20261017):
    """n (tracker, k_commitment, k, blinder) tuples as concatenated byte strings: r_G = r G, k_r_G = k r_G, k_G = k G on the GPU"""
    rng = random.Random(seed)
    ks, rs, bs = (params.random_fr_wire(rng, n) for _ in range(3))
    one = params.fp_to_wire(1)
    comp = lambda aff: ctx.normalize(b"".join(aff[96 * i:96 * (i + 1)] + one for i in range(n)), compressed=True)[1]
    gens = params.g1_generator_wire() * n
    r_g = ctx.scale(gens, rs)
    cr, ckr, ck = comp(r_g), comp(ctx.scale(r_g, ks)), comp(ctx.scale(gens, ks))
    trackers = b"".join(cr[48 * i:48 * (i + 1)] + ckr[48 * i:48 * (i + 1)] for i in range(n))
    return trackers, ck, ks, bs


def median_seconds(fn, runs):
    fn()   # warm-up
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="64,1024,16384")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--single", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    counts = [int(c) for c in a.counts.split(",")]
    nmax = max(counts + [a.single])
    ctx = cpx.Context(0)
    L, h = ctx._L, ctx._h
    trackers, kcs, ks, bs = make_inputs(ctx, nmax)
    res = {"counts": counts, "runs": a.runs, "batched": {}, "kernel_ms": {}}
    ok = True
    proofs_all = None
    for n in sorted(counts, reverse=True):
        tr, kc, k, b = (cpx._in(x) for x in (trackers[:96 * n], kcs[:48 * n], ks[:32 * n], bs[:32 * n]))
        out, st = cpx._out(128 * n), (ctypes.c_int * n)()
        gen = lambda: ctx._check(L.cpx_whisk_generate_tracker_proofs(h, n, tr, k, b, out, st))
        t_gen = median_seconds(gen, a.runs)
        ok &= all(s == cpx.CPX_OK for s in st)
        if proofs_all is None:
            proofs_all = bytes(out)
        verdict = (ctypes.c_int * n)()
        ver = lambda: ctx._check(L.cpx_whisk_verify_tracker_proofs(h, n, tr, kc, out, verdict))
        t_ver = median_seconds(ver, a.runs)
        ok &= all(v == cpx.CPX_OK for v in verdict)
        res["batched"][n] = {"verify_s": t_ver, "verify_per_s": n / t_ver, "generate_s": t_gen, "generate_per_s": n / t_gen}
        ctx.set_profiling(True)
        ctx.reset_stats()
        ver()
        kv = {k_: ctx.stat(k_)["ms"] for k_ in KERNELS[:3]}
        ctx.reset_stats()
        gen()
        kg = {k_: ctx.stat(k_)["ms"] for k_ in KERNELS if k_ != "k_tracker_relations"}
        ctx.set_profiling(False)
        res["kernel_ms"][n] = {"verify": kv, "generate": kg}
    # the single-proof calls, one item after the other (their code is the parent commit's)
    m = a.single
    items = [(cpx._in(trackers[96 * i:96 * (i + 1)]), cpx._in(kcs[48 * i:48 * (i + 1)]), cpx._in(ks[32 * i:32 * (i + 1)]), cpx._in(bs[32 * i:32 * (i + 1)]),
              cpx._in(proofs_all[128 * i:128 * (i + 1)]), cpx._out(128)) for i in range(m)]
    valid = ctypes.c_int(0)

    def single_verify():
        for tr, kc, _, _, pf, _ in items:
            ctx._check(L.cpx_whisk_is_valid_tracker_proof(h, tr, kc, pf, ctypes.byref(valid)))
            assert valid.value == 1

    def single_generate():
        for tr, _, k, b, _, o in items:
            ctx._check(L.cpx_whisk_generate_tracker_proof(h, tr, k, b, o))

    t_sv, t_sg = median_seconds(single_verify, a.runs), median_seconds(single_generate, a.runs)
    ok &= all(bytes(it[5]) == proofs_all[128 * i:128 * (i + 1)] for i, it in enumerate(items))
    res["single_loop"] = {"items": m, "verify_s": t_sv, "verify_per_s": m / t_sv, "generate_s": t_sg, "generate_per_s": m / t_sg}
    res["speedup_vs_single_loop"] = {n: {"verify": r["verify_per_s"] / (m / t_sv), "generate": r["generate_per_s"] / (m / t_sg)} for n, r in res["batched"].items()}
    res["all_results_as_expected"] = bool(ok)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
