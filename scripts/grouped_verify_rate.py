"""What naming the wrong proofs costs: cpx_batch_verify, cpx_batch_verify_fused and cpx_batch_verify_grouped on the same loaded batch, one context.

    python scripts/grouped_verify_rate.py [--ell 252] [--batches 8192,1024] [--wrong 0,1,8,256] [--runs 5] [--groups-max 256] [--out FILE.md]

For every batch size: one instance (seeded; made with cpx_batch_shuffle and proved with cpx_batch_prove) repeated over the batch, every proof
with factors of its own.  Then, for every count of wrong proofs (a proof whose z_k is off by one: only the SameScalar equalities fail), the
wrong proofs spread over distinct groups: the median host-clock time of --runs calls of each verifier after one warm-up call, at the C-ABI
with the buffers marshalled beforehand, and the grouped call's n_rechecked beside its time.  Exit status 1 if a verdict is not what the
mutation implies or the three calls disagree.
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

SEED = "grouped_verify_rate"
R_ = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def z_k_offset(ell):
    """byte offset of z_k inside CurdleproofsProof::serialize (curdleproofs.rs:300-310): nine points, r_p, B_c B_d and the 4 L IPA points,
    c d, the four SameScalar commitments"""
    L = (ell + 4).bit_length() - 1
    return 9 * 48 + 32 + (2 + 4 * L) * 48 + 64 + 4 * 48


def timed(fn, runs):
    fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ell", type=int, default=252)
    ap.add_argument("--batches", default="8192,1024")
    ap.add_argument("--wrong", default="0,1,8,256")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--groups-max", type=int, default=256)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = cpx.Context(0, options={"locate_groups_max": a.groups_max})
    L, h = ctx._L, ctx._h
    ell, n = a.ell, a.ell + 4
    crsmod.crs_from_seed(ctx, ell, SEED)
    psz = ctx.proof_size
    rng = random.Random(20261019)
    vec_r = ctx.scale(params.g1_generator_wire() * ell, params.random_fr_wire(rng, ell))
    vec_s = ctx.scale(vec_r, params.random_fr_wire(rng, ell))
    perm = list(range(ell))
    rng.shuffle(perm)
    k, mb, draws = params.random_fr_wire(rng, 1), params.random_fr_wire(rng, 4), params.random_fr_wire(rng, 3 * n + 9)
    vec_t, vec_u, m = ctx.shuffle_batch(vec_r, vec_s, perm, k, mb)
    good = ctx.prove_batch(perm, k, mb, draws)[0]
    o = z_k_offset(ell)
    bad = good[:o] + ((int.from_bytes(good[o:o + 32], "little") + 1) % R_).to_bytes(32, "little") + good[o + 32:]
    ok = True
    say("# grouped_verify_rate: ell = %d, proof %d B, runs = %d (median, host clock), locate_groups_max = %d, device_min_batch = %d, fix_bits = %d" %
        (ell, psz, a.runs, a.groups_max, ctx.get_option("device_min_batch"), ctx.get_option("fix_bits_effective")))
    say("")
    say("| batch | wrong | `cpx_batch_verify` ms | proofs/s | `cpx_batch_verify_fused` ms | proofs/s | `cpx_batch_verify_grouped` ms | proofs/s | n_rechecked | grouped / fused |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    for B in (int(b) for b in a.batches.split(",")):
        ctx.load_batch(vec_r * B, vec_s * B, vec_t * B, vec_u * B, m * B)
        rand8, rand12 = cpx._in(params.random_fr_wire(rng, 8 * B)), cpx._in(params.random_fr_wire(rng, 12 * B))
        G = -(-B // a.groups_max)
        NT = -(-B // G)
        for nw in (int(w) for w in a.wrong.split(",")):
            if nw > NT:
                continue
            victims = sorted({(i * NT // nw) * G for i in range(nw)}) if nw else []
            blob = bytearray(good * B)
            for p in victims:
                blob[p * psz:(p + 1) * psz] = bad
            proofs = cpx._in(bytes(blob))
            want = [cpx.CPX_ERR_VERIFY if p in set(victims) else cpx.CPX_OK for p in range(B)]
            v8, v12 = (ctypes.c_int * B)(), (ctypes.c_int * B)()
            part, nbad, rechecked = cpx._out(144), ctypes.c_int(0), ctypes.c_size_t(0)
            t_per = timed(lambda: ctx._check(L.cpx_batch_verify(h, proofs, rand8, v8)), a.runs)
            t_fus = timed(lambda: ctx._check(L.cpx_batch_verify_fused(h, proofs, rand12, part, ctypes.byref(nbad))), a.runs)
            t_grp = timed(lambda: ctx._check(L.cpx_batch_verify_grouped(h, proofs, rand12, v12, ctypes.byref(rechecked))), a.runs)
            accepted = nbad.value == 0 and ctx.sum_jac(bytes(part)[:144])[1]
            ok &= list(v8) == want and list(v12) == want and accepted == (nw == 0)
            ok &= rechecked.value == sum(min(G, B - p) for p in victims)
            say("| %d | %d | %.2f | %.0f | %.2f | %.0f | %.2f | %.0f | %d | %.3f |" %
                (B, nw, 1e3 * t_per, B / t_per, 1e3 * t_fus, B / t_fus, 1e3 * t_grp, B / t_grp, rechecked.value, t_grp / t_fus))
    say("")
    say("all verdicts as expected: %s" % bool(ok))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
