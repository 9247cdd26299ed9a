"""What the log-round loops cost as ONE call each (cpx_ipa_rounds, cpx_same_msm_rounds) against the per-round route of tier 0.

    python scripts/loop_rounds_timing.py [--runs 20] [--out FILE]

One context, n = 256 (the 8 rounds of either argument at ell = 252), count = 1, 16 and 256 independent items.  Both loops go two ways,
in the same process, runs alternating, 3 warm-up runs, then the median of `--runs` runs on the host clock:
  one call    the whole loop of all items in cpx_ipa_rounds / cpx_same_msm_rounds: one synchronisation
  per round   scripts/tier0_round_timing.py's route for all items at once: per round one cpx_g1_msm_many over the count x 4 (6) cross
              terms, the host transcript of every item between the calls (cpx_transcript_append_message x 4 (6) and
              cpx_transcript_challenge_scalar on the round's real encodings), one cpx_g1_fold_many over the count x 2 (3) families with
              the challenges just drawn: 16 synchronisations.  Its buffers are marshalled beforehand with the sizes of every round (the
              time of an MSM or a fold does not depend on the values), and the scalar folds a caller does on its own are left out, so the
              figure is the library's share of that route plus the transcript calls, which are reported on their own as well.
Points are multiples of the generator by seeded scalars.  A record, not a threshold: no test depends on a time.
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

FR, AFF, ST = 32, 96, 216
N, LOG_N = 256, 8
COUNTS = (1, 16, 256)
WARMUP = 3
SHAPES = {"IPA": dict(terms=4, fams=2, nvec=2, loop=b"ipa_loop", gamma=b"ipa_gamma"),
          "SameMSM": dict(terms=6, fams=3, nvec=1, loop=b"same_msm_loop", gamma=b"same_msm_gamma")}


class Loop:
    def __init__(self, ctx, kind, count, points, scalars):
        self.ctx, self.L, self.h, self.kind, self.count = ctx, ctx._L, ctx._h, kind, count
        sh = self.sh = SHAPES[kind]
        take = lambda buf, each, k: cpx._in((buf * (k * each // len(buf) + 1))[:k * each])      # k elements, the pool repeated
        # ---- one call
        self.fn = self.L.cpx_ipa_rounds if kind == "IPA" else self.L.cpx_same_msm_rounds
        ins = [take(points, AFF, count * N), take(points[AFF * 7:] + points[:AFF * 7], AFF, count * N)]
        ins += [take(points, AFF, count)] if kind == "IPA" else [take(points[AFF * 13:] + points[:AFF * 13], AFF, count * N)]
        ins += [take(scalars[FR * v:] + scalars[:FR * v], FR, count * N) for v in range(sh["nvec"])]
        self.ins = ins
        self.state0 = Transcript.new(b"loop_rounds_timing").state * count
        self.states = cpx._out(ST * count)
        self.comp, self.fin, self.gam = cpx._out(count * LOG_N * sh["terms"] * 48), cpx._out(count * sh["nvec"] * FR), cpx._out(count * LOG_N * FR)
        # ---- per round: the sizes of every round
        self.rounds = []
        for j in range(LOG_N):
            half = N >> (j + 1)
            lens = [half + 1, half, half + 1, half] if kind == "IPA" else [half] * 6
            npts = sum(lens) * count
            self.rounds.append(dict(half=half, ntasks=len(lens) * count, lens=(ctypes.c_uint32 * (len(lens) * count))(*(lens * count)),
                                    bases=take(points, AFF, npts), scalars=take(scalars, FR, npts), out=cpx._out(48 * len(lens) * count),
                                    pl=take(points, AFF, sh["fams"] * count * half), pr=take(points[AFF * 5:] + points[:AFF * 5], AFF, sh["fams"] * count * half),
                                    gammas=cpx._out(FR * sh["fams"] * count)))
        self.t_transcript = 0.0

    def one_call(self):
        ctypes.memmove(self.states, self.state0, ST * self.count)
        self.ctx._check(self.fn(self.h, self.count, N, *self.ins, self.states, self.comp, None, self.fin, self.gam))

    def per_round(self):
        sh, L = self.sh, self.L
        states = [(ctypes.c_uint8 * ST).from_buffer_copy(self.state0[:ST]) for _ in range(self.count)]
        g = (ctypes.c_uint8 * FR)()
        for r in self.rounds:
            self.ctx._check(L.cpx_g1_msm_many(self.h, r["ntasks"], r["lens"], r["bases"], r["scalars"], None, r["out"]))
            t0 = time.perf_counter()
            enc = bytes(r["out"])
            for i, st in enumerate(states):
                for q in range(sh["terms"]):
                    o = 48 * (i * sh["terms"] + q)
                    L.cpx_transcript_append_message(st, sh["loop"], len(sh["loop"]), enc[o:o + 48], 48)
                L.cpx_transcript_challenge_scalar(st, sh["gamma"], len(sh["gamma"]), g)
                for f in range(sh["fams"]):                      # (the IPA folds G' by the inverse: another scalar, the same cost)
                    ctypes.memmove(ctypes.addressof(r["gammas"]) + FR * (i * sh["fams"] + f), g, FR)
            self.t_transcript += time.perf_counter() - t0
            self.ctx._check(L.cpx_g1_fold_many(self.h, sh["fams"] * self.count, r["half"], r["pl"], r["pr"], r["gammas"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = cpx.Context(0)
    rnd = random.Random(20261020)
    pool = 2048
    scalars = params.random_fr_wire(rnd, pool)
    points = ctx.generator_mul(params.random_fr_wire(rnd, pool))
    lines = ["log-round loops at n = %d (%d rounds), one context, runs alternating, median of %d runs after %d warm-up runs, ms per loop over all items"
             % (N, LOG_N, a.runs, WARMUP),
             "%-8s %6s | %10s %10s | %10s %14s %8s" % ("loop", "count", "one call", "per item", "per round", "of it transcr.", "ratio")]
    for kind in SHAPES:
        for count in COUNTS:
            lp = Loop(ctx, kind, count, points, scalars)
            for _ in range(WARMUP):
                lp.one_call()
                lp.per_round()
            lp.t_transcript = 0.0
            t_one, t_round = [], []
            for _ in range(a.runs):
                for fn, acc in ((lp.one_call, t_one), (lp.per_round, t_round)):
                    t0 = time.perf_counter()
                    fn()
                    acc.append(time.perf_counter() - t0)
            one, rnds = 1e3 * statistics.median(t_one), 1e3 * statistics.median(t_round)
            lines.append("%-8s %6d | %10.3f %10.4f | %10.3f %14.3f %8.2f" % (kind, count, one, one / count, rnds, 1e3 * lp.t_transcript / a.runs, rnds / one))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
