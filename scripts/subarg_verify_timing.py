"""What the stand-alone sub-argument verifiers cost as ONE call each (cpx_ipa_verify, cpx_same_msm_verify) against the bare
multi-scalar multiplication any host-driven route has to run as well.

    python scripts/subarg_verify_timing.py [--runs 20] [--out FILE]

One context, n = 256, count = 1, 16 and 256 independent items.  Two routes in the same process, runs alternating, 3 warm-up runs, then the
median of `--runs` runs on the host clock:
  one call   cpx_ipa_verify / cpx_same_msm_verify over all items: decoding, the transcripts, the weights and the MSM, one synchronisation
  MSM alone  cpx_g1_msm_many with one task per item over the SAME points (n + 4 L + 5 resp. 3 n + 6 L + 6 of them, already affine) and
             scalars that the host has computed beforehand: what is left of the accumulator route (cpx_accum_check, cpx_accum_verify)
             when the host's transcript replay, inversions, O(n log n) field products and decoding cost nothing — a lower bound for any
             host-driven route.  The call exists without the verifiers, so it is the yardstick, not the code under test.
The proof points are valid encodings and the scalars seeded values; the proofs are not valid ones (the time of neither route depends on the
verdict: a rejected item runs the same launches).  The time of k_subarg_scalars alone comes from Context.stats() in a profiled pass after
the timed runs.  A record, not a threshold: no test depends on a time.
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
from curdleproofs_amd import params   # noqa: E402
from curdleproofs_amd.transcript import Transcript   # noqa: E402

FR, AFF, JAC, ST = 32, 96, 144, 216
N, LOG_N = 256, 8
COUNTS = (1, 16, 256)
WARMUP = 3
FP_ONE = bytes.fromhex("fdff02000000097602000cc40b00f4ebba58c7535798485f455752705358ce776dec56a2971a075c93e480fac35ef615")   # R mod p, 12 x u32 LE
SHAPES = {"IPA": dict(fams=1, pp=2 + 4 * LOG_N, nsc=2, checks=2), "SameMSM": dict(fams=3, pp=3 + 6 * LOG_N, nsc=1, checks=3)}


class Case:
    def __init__(self, ctx, kind, count, aff, comp, scalars):
        self.ctx, self.L, self.h, self.kind, self.count = ctx, ctx._L, ctx._h, kind, count
        sh = SHAPES[kind]
        take = lambda buf, each, k, skip=0: ((buf[each * skip:] + buf[:each * skip]) * (k * each // len(buf) + 1))[:k * each]   # k elements, the pool repeated
        jac = lambda k, skip: b"".join(take(aff, AFF, k, skip)[AFF * i:AFF * (i + 1)] + FP_ONE for i in range(k))
        canon = (123456789).to_bytes(FR, "little")                        # a canonical scalar of a proof
        proof = lambda i: take(comp, 48, sh["pp"], 3 * i) + canon * sh["nsc"]
        self.fn = self.L.cpx_ipa_verify if kind == "IPA" else self.L.cpx_same_msm_verify
        pts = [take(aff, AFF, count * N, 5 * f) for f in range(sh["fams"])]
        stmt = [jac(count, 11 + k) for k in range(3)]
        fr = [take(scalars, FR, count), take(scalars, FR, count * N, 9)] if kind == "IPA" else []
        self.ins = [cpx._in(b) for b in (pts[:1] + stmt + fr if kind == "IPA" else pts + stmt)]
        self.ins += [cpx._in(b"".join(proof(i) for i in range(count))), cpx._in(take(scalars, FR, count * sh["checks"], 17))]
        self.state0 = Transcript.new(b"subarg_verify_timing").state * count
        self.states, self.verdicts = cpx._out(ST * count), (ctypes.c_int * count)()
        # ---- the MSM alone: one task per item over as many points, scalars ready
        per = sh["fams"] * N + sh["pp"] + 3
        self.lens = (ctypes.c_uint32 * count)(*([per] * count))
        self.bases, self.scal, self.out = cpx._in(take(aff, AFF, count * per)), cpx._in(take(scalars, FR, count * per)), cpx._out(JAC * count)

    def one_call(self):
        ctypes.memmove(self.states, self.state0, ST * self.count)
        self.ctx._check(self.fn(self.h, self.count, N, *self.ins, self.states, None, self.verdicts))

    def msm_alone(self):
        self.ctx._check(self.L.cpx_g1_msm_many(self.h, self.count, self.lens, self.bases, self.scal, self.out, None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = cpx.Context(0)
    rnd = random.Random(20261020)
    pool = 2048
    scalars = params.random_fr_wire(rnd, pool)
    aff, comp = ctx.generator_mul(params.random_fr_wire(rnd, pool), compressed=True)
    lines = ["sub-argument verifiers at n = %d, one context, runs alternating, median of %d runs after %d warm-up runs, ms per call over all items"
             % (N, a.runs, WARMUP),
             "%-8s %6s | %10s %10s | %10s %10s | %8s %16s" % ("verifier", "count", "one call", "per item", "MSM alone", "per item", "ratio", "k_subarg_scalars")]
    for kind in SHAPES:
        for count in COUNTS:
            c = Case(ctx, kind, count, aff, comp, scalars)
            for _ in range(WARMUP):
                c.one_call()
                c.msm_alone()
            assert all(v in (cpx.CPX_OK, cpx.CPX_ERR_VERIFY) for v in c.verdicts)      # every item decoded: the full chain ran
            t_one, t_msm = [], []
            for _ in range(a.runs):
                for fn, acc in ((c.one_call, t_one), (c.msm_alone, t_msm)):
                    t0 = time.perf_counter()
                    fn()
                    acc.append(time.perf_counter() - t0)
            ctx.set_profiling(True)
            ctx.reset_stats()
            for _ in range(5):
                c.one_call()
            st = ctx.stat("k_subarg_scalars")
            ctx.set_profiling(False)
            one, msm = 1e3 * statistics.median(t_one), 1e3 * statistics.median(t_msm)
            lines.append("%-8s %6d | %10.3f %10.4f | %10.3f %10.4f | %8.2f %13.3f ms" % (kind, count, one, one / count, msm, msm / count, one / msm, st["ms"] / max(st["launches"], 1)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
