"""What a log round costs through tier 0: call by call (cpx_g1_msm, cpx_g1_fold) against one cpx_g1_msm_many + one cpx_g1_fold_many.

    python scripts/tier0_round_timing.py [--runs 20] [--out FILE]

On one context, for half = 128, 64, ..., 1 — the 8 rounds of either argument at ell = 252 — two shapes are timed both ways:
  IPA      4 MSMs of (half + 1, half, half + 1, half) points (inner_product_argument.rs:158-161, H appended to the bases of L_C and R_C)
           and 2 folds of half elements (:177-178)
  SameMSM  6 MSMs of half points (same_multiscalar_argument.rs:107-112) and 3 folds of half elements (:128-130)
Every shape: 3 warm-up runs, then the median of `--runs` runs, host clock around calls that each end in a stream synchronisation.  Buffers
are marshalled beforehand, so the figures are the library's, not ctypes'.  Points are multiples of the generator by seeded scalars.  The
table ends with the sum over the 16 rounds.  Below it, the A/B behind option fold_quad_max: cpx_g1_fold_many of 3 x 128 and 3 x 512
elements as k_smul_quad (fold_quad_max above the size) and as the one-lane k_smul (fold_quad_max = 0), runs alternating.  A record, not a
threshold: no test depends on a time.
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

FR, AFF, JAC = 32, 96, 144
HALVES = (128, 64, 32, 16, 8, 4, 2, 1)
WARMUP = 3


def median_ms(fn, runs):
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(t)


class Round:
    """the marshalled buffers of one round shape, and its two ways through the library"""

    def __init__(self, ctx, points, scalars, lens, families, half):
        self.ctx, self.L, self.h = ctx, ctx._L, ctx._h
        self.lens, self.families, self.half = lens, families, half
        off, self.msm_in = 0, []
        for n in lens:                                   # consecutive ranges of the pool: no two tasks alike
            self.msm_in.append((cpx._in(points[AFF * off:AFF * (off + n)]), cpx._in(scalars[FR * off:FR * (off + n)]), n))
            off += n
        npts = sum(lens)
        self.bases, self.scalars = cpx._in(points[:AFF * npts]), cpx._in(scalars[:FR * npts])
        self.lens_arr = (ctypes.c_uint32 * len(lens))(*lens)
        self.out1, self.out_many = cpx._out(JAC), cpx._out(JAC * len(lens))
        self.pl = [cpx._in(points[AFF * (300 * f):AFF * (300 * f + half)]) for f in range(families)]
        self.pr = [cpx._in(points[AFF * (300 * f + 150):AFF * (300 * f + 150 + half)]) for f in range(families)]
        self.gam = [cpx._in(scalars[FR * f:FR * (f + 1)]) for f in range(families)]
        self.pl_many = cpx._in(b"".join(bytes(b)[:AFF * half] for b in self.pl))
        self.pr_many = cpx._in(b"".join(bytes(b)[:AFF * half] for b in self.pr))
        self.gam_many = cpx._in(scalars[:FR * families])

    # (the folds run in place on their own output: every run folds other points, none of them special)
    def single(self):
        for b, s, n in self.msm_in:
            self.ctx._check(self.L.cpx_g1_msm(self.h, b, s, n, self.out1))
        for f in range(self.families):
            self.ctx._check(self.L.cpx_g1_fold(self.h, self.pl[f], self.pr[f], self.gam[f], self.half))

    def many(self):
        self.ctx._check(self.L.cpx_g1_msm_many(self.h, len(self.lens), self.lens_arr, self.bases, self.scalars, self.out_many, None))
        self.ctx._check(self.L.cpx_g1_fold_many(self.h, self.families, self.half, self.pl_many, self.pr_many, self.gam_many))

    def fold_many_only(self):
        self.ctx._check(self.L.cpx_g1_fold_many(self.h, self.families, self.half, self.pl_many, self.pr_many, self.gam_many))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = cpx.Context(0)
    rnd = random.Random(20261019)
    pool = 2048
    scalars = params.random_fr_wire(rnd, pool)
    points = ctx.generator_mul(params.random_fr_wire(rnd, pool))
    lines = ["tier-0 log rounds, one context, median of %d runs after %d warm-up runs, ms per round (fold_quad_max = %d)"
             % (a.runs, WARMUP, ctx.get_option("fold_quad_max")),
             "%5s | %-34s | %-34s" % ("", "IPA: 4 MSMs + 2 folds", "SameMSM: 6 MSMs + 3 folds"),
             "%5s | %10s %10s %10s | %10s %10s %10s" % ("half", "6 calls", "2 calls", "ratio", "9 calls", "2 calls", "ratio")]
    total = [0.0] * 4
    for half in HALVES:
        ipa = Round(ctx, points, scalars, (half + 1, half, half + 1, half), 2, half)
        smsm = Round(ctx, points, scalars, (half,) * 6, 3, half)
        t = [median_ms(ipa.single, a.runs), median_ms(ipa.many, a.runs), median_ms(smsm.single, a.runs), median_ms(smsm.many, a.runs)]
        total = [x + y for x, y in zip(total, t)]
        lines.append("%5d | %10.3f %10.3f %10.2f | %10.3f %10.3f %10.2f" % (half, t[0], t[1], t[0] / t[1], t[2], t[3], t[2] / t[3]))
    lines.append("%5s | %10.3f %10.3f %10.2f | %10.3f %10.3f %10.2f" % ("sum", total[0], total[1], total[0] / total[1], total[2], total[3], total[2] / total[3]))
    lines.append("16 rounds (8 IPA + 8 SameMSM): %.2f ms call by call (120 calls), %.2f ms per round (32 calls)" % (total[0] + total[2], total[1] + total[3]))
    lines.append("")
    lines.append("cpx_g1_fold_many, 3 families: quad per element (fold_quad_max = 2^20) against one lane per element (fold_quad_max = 0), %d alternating runs" % a.runs)
    for half in (128, 512):
        r = Round(ctx, points, scalars, (1,), 3, half)
        t_quad, t_lane = [], []
        for q in (1 << 20, 0):                            # warm-up of both forms
            ctx.set_option("fold_quad_max", q)
            r.fold_many_only()
        for _ in range(a.runs):
            for q, acc in ((1 << 20, t_quad), (0, t_lane)):
                ctx.set_option("fold_quad_max", q)
                t0 = time.perf_counter()
                r.fold_many_only()
                acc.append(time.perf_counter() - t0)
        mq, ml = 1e3 * statistics.median(t_quad), 1e3 * statistics.median(t_lane)
        lines.append("3 x %3d = %4d elements: k_smul_quad %.3f ms (min %.3f max %.3f), k_smul %.3f ms (min %.3f max %.3f), one lane / quad %.2f"
                     % (half, 3 * half, mq, 1e3 * min(t_quad), 1e3 * max(t_quad), ml, 1e3 * min(t_lane), 1e3 * max(t_lane), ml / mq))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
