"""What SamePermutationProof::new and ::verify cost as ONE call each (cpx_same_perm_prove, cpx_same_perm_verify) against the composed routes
a caller of the stand-alone API had before them, on the same build.

    python scripts/same_perm_timing.py [--runs 20] [--out FILE]

n = 128 and n = 256 with n_blinders = 4 (ell = 124 and 252), count = 1 and 256 independent items, runs alternating, 3 warm-up runs, then the
median of `--runs` runs on the host clock with the smallest and the largest run beside it:
  one call   the whole `new` of all items in cpx_same_perm_prove on explicit draws: one synchronisation
  composed   item by item: step 1 through cpx_transcript_* (A, M, then vec_a as one message), the factors, their product and vec_b_blinders
             on the host, B = A + alpha M + beta sum G through ONE Context.msm over G | M | A; then ONE Context.gprod_prove over all items.
             The host's Fr arithmetic is Python integers here (a Rust caller's is some hundred times faster), so its share is reported on
             its own, as is the transcript's; "device calls" is the composed route without either.
Before anything is timed the two routes' proof bytes and end states are compared for every item: they must be equal.
The verifier likewise, on the proofs the prover made:
  one call   cpx_same_perm_verify over all items: one synchronisation
  composed   per item step 1 through cpx_transcript_*, gprod_result on the host, the relation of same_permutation_argument.rs:149 as ONE
             Context.msm over G | B | A | M whose sum must be the identity; then ONE Context.gprod_verify over all items.
Both must give the same verdicts (all accepted) and end states.  The per-kernel times of k_same_perm_step / k_same_perm_verify_step /
k_same_perm_weights come from one profiled call per shape (Context.stat).  Points are multiples of the generator by seeded scalars.  A
record, not a threshold: no test depends on a time.
"""
import argparse
import os
import random
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import curdleproofs_amd as cpx   # noqa: E402
from curdleproofs_amd import params   # noqa: E402
from curdleproofs_amd.params import R, fr_from_wire, fr_to_wire   # noqa: E402
from curdleproofs_amd.transcript import Transcript   # noqa: E402

FR, AFF, JAC, ST = 32, 96, 144, 216
SHAPES = ((124, 4), (252, 4))
COUNTS = (1, 256)
WARMUP = 3
wire = lambda v: b"".join(fr_to_wire(x % R) for x in v)


class Case:
    def __init__(self, ctx, ell, nb, count, points, rnd):
        self.ctx, self.ell, self.nb, self.count = ctx, ell, nb, count
        n = self.n = ell + nb
        rot = lambda k: (points[AFF * k:] + points[:AFF * k])
        take = lambda buf, each, k: (buf * (k * each // len(buf) + 1))[:k * each]
        one = params.fp_to_wire(1)
        self.jac = jac = lambda aff: b"".join(aff[AFF * i:AFF * (i + 1)] + (one if aff[AFF * i:AFF * (i + 1)] != bytes(AFF) else bytes(48)) for i in range(len(aff) // AFF))
        self.G, self.H = take(rot(0), AFF, count * ell), take(rot(900), AFF, count * nb)
        self.U = jac(take(rot(100), AFF, count))
        self.a_int = [rnd.randrange(1, R) for _ in range(count * ell)]
        self.ra_int = [rnd.randrange(1, R) for _ in range(count * nb)]
        self.rm_int = [rnd.randrange(1, R) for _ in range(count * nb)]
        self.perm = []
        for _ in range(count):
            p = list(range(ell))
            rnd.shuffle(p)
            self.perm += p
        # a statement the witness satisfies (same_permutation_argument.rs:216-240)
        A, M = [], []
        for i in range(count):
            GH = self.GH(i)
            a, p = self.a_int[ell * i:ell * (i + 1)], self.perm[ell * i:ell * (i + 1)]
            A.append(ctx.normalize(ctx.msm(GH, wire([a[s] for s in p] + self.ra_int[nb * i:nb * (i + 1)]))))
            M.append(ctx.normalize(ctx.msm(GH, wire(p + self.rm_int[nb * i:nb * (i + 1)]))))
        self.A_aff, self.M_aff = b"".join(A), b"".join(M)
        self.A, self.M = jac(self.A_aff), jac(self.M_aff)
        self.A_comp, self.M_comp = ctx.normalize(self.A, compressed=True)[1], ctx.normalize(self.M, compressed=True)[1]   # what step 1 hashes: a caller has them
        self.a, self.ra, self.rm = wire(self.a_int), wire(self.ra_int), wire(self.rm_int)
        self.perm_bytes = struct.pack("<%dI" % len(self.perm), *self.perm)
        self.msgs = [ell.to_bytes(8, "little") + b"".join(x.to_bytes(32, "little") for x in self.a_int[ell * i:ell * (i + 1)]) for i in range(count)]
        self.de = nb + 2 * n - 2
        self.draws = wire([rnd.randrange(1, R) for _ in range(count * self.de)])
        self.state0 = Transcript.new(b"same_perm_timing").state
        ones = fr_to_wire(1)
        sums = lambda pts, each: b"".join(ctx.normalize(ctx.msm(pts[AFF * each * i:AFF * each * (i + 1)], ones * each)) if each else bytes(AFF) for i in range(count))
        self.g_sum, self.h_sum = sums(self.G, ell), sums(self.H, nb)       # the CRS sums: a verifier has them
        self.vrand = wire([rnd.randrange(1, R) for _ in range(3 * count)])
        self.proofs = None
        self.t_host = self.t_transcript = 0.0

    def GH(self, i):
        return self.G[AFF * self.ell * i:AFF * self.ell * (i + 1)] + self.H[AFF * self.nb * i:AFF * self.nb * (i + 1)]

    def step1(self, i):
        t0 = time.perf_counter()
        t = Transcript.from_state(self.state0)
        t.append_message(b"same_perm_step1", self.A_comp[48 * i:48 * (i + 1)])
        t.append_message(b"same_perm_step1", self.M_comp[48 * i:48 * (i + 1)])
        t.append_message(b"same_perm_step1", self.msgs[i])
        alpha, beta = fr_from_wire(t.challenge_scalar(b"same_perm_alpha")), fr_from_wire(t.challenge_scalar(b"same_perm_beta"))
        self.t_transcript += time.perf_counter() - t0
        return t, alpha, beta

    def one_call(self):
        out = self.ctx.same_perm_prove(self.ell, self.G, self.H, self.U, self.A, self.M, self.a, self.perm_bytes, self.ra, self.rm, self.state0 * self.count, rand=self.draws)
        assert all(s is True for s in out["status"])
        return b"".join(out["proofs"]), out["states"]

    def composed(self):
        ctx, ell, nb, count = self.ctx, self.ell, self.nb, self.count
        Bs, res, bs, rbs, states, heads = [], [], [], [], [], []
        for i in range(count):
            t, alpha, beta = self.step1(i)
            t0 = time.perf_counter()
            a, p = self.a_int[ell * i:ell * (i + 1)], self.perm[ell * i:ell * (i + 1)]
            f = [(a[s] + s * alpha + beta) % R for s in p]
            prod = 1
            for x in f:
                prod = prod * x % R
            rb = [(x + alpha * y) % R for x, y in zip(self.ra_int[nb * i:nb * (i + 1)], self.rm_int[nb * i:nb * (i + 1)])]
            sc = wire([beta] * ell + [alpha, 1])
            self.t_host += time.perf_counter() - t0
            B = ctx.msm(self.G[AFF * ell * i:AFF * ell * (i + 1)] + self.M_aff[AFF * i:AFF * (i + 1)] + self.A_aff[AFF * i:AFF * (i + 1)], sc)
            Bs.append(B), res.append(fr_to_wire(prod)), bs.append(wire(f)), rbs.append(wire(rb)), states.append(t.state)
            heads.append(ctx.normalize(B, compressed=True)[1])
        cat = b"".join
        out = ctx.gprod_prove(ell, self.G, self.H, self.U, cat(Bs), cat(res), cat(bs), cat(rbs), cat(states), rand=self.draws)
        return cat(h + p for h, p in zip(heads, out["proofs"])), out["states"]

    def verify_one(self):
        out = self.ctx.same_perm_verify(self.ell, self.G, self.H, self.U, self.g_sum, self.h_sum, self.A, self.M, self.a, self.proofs, self.vrand, self.state0 * self.count)
        return out["verdicts"], out["states"]

    def verify_composed(self):
        ctx, ell, count = self.ctx, self.ell, self.count
        pb = len(self.proofs) // count
        Bs, res, states, inner, rel = [], [], [], [], []
        for i in range(count):
            proof = self.proofs[pb * i:pb * (i + 1)]
            t, alpha, beta = self.step1(i)
            t0 = time.perf_counter()
            prod = 1
            for k, x in enumerate(self.a_int[ell * i:ell * (i + 1)]):
                prod = prod * (x + k * alpha + beta) % R
            sc = wire([beta] * ell + [-1, 1, alpha])
            self.t_host += time.perf_counter() - t0
            B_aff = ctx.decompress(proof[:48])
            O = ctx.msm(self.G[AFF * ell * i:AFF * ell * (i + 1)] + B_aff + self.A_aff[AFF * i:AFF * (i + 1)] + self.M_aff[AFF * i:AFF * (i + 1)], sc)
            rel.append(ctx.normalize(O) == bytes(AFF))                     # same_permutation_argument.rs:149 on its own
            Bs.append(self.jac(B_aff)), res.append(fr_to_wire(prod)), states.append(t.state), inner.append(proof[48:])
        cat = b"".join
        vr = cat(self.vrand[FR * (3 * i + 1):FR * (3 * i + 3)] for i in range(count))
        out = ctx.gprod_verify(ell, self.G, self.H, self.U, self.g_sum, self.h_sum, cat(Bs), cat(res), cat(inner), vr, cat(states))
        return [v is True and r for v, r in zip(out["verdicts"], rel)], out["states"]


def measure(case, one, comp, runs):
    for _ in range(WARMUP):
        one()
        comp()
    case.t_host = case.t_transcript = 0.0
    t_one, t_comp = [], []
    for _ in range(runs):
        for fn, acc in ((one, t_one), (comp, t_comp)):
            t0 = time.perf_counter()
            fn()
            acc.append(1e3 * (time.perf_counter() - t0))
    m1, mc = statistics.median(t_one), statistics.median(t_comp)
    host, tr = 1e3 * case.t_host / runs, 1e3 * case.t_transcript / runs
    return "%9.3f (%7.3f .. %7.3f) %10.4f | %10.3f (%8.3f .. %8.3f) %10.3f %12.3f %12.3f | %8.2f %8.2f" % (
        m1, min(t_one), max(t_one), m1 / case.count, mc, min(t_comp), max(t_comp), host, tr, mc - host - tr, mc / m1, (mc - host - tr) / m1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = cpx.Context(0)
    rnd = random.Random(20261021)
    points = ctx.generator_mul(params.random_fr_wire(rnd, 2048))
    head = "%5s %6s | %28s %10s | %30s %10s %12s %12s | %8s %8s | %s" % ("n", "count", "one call", "per item", "composed", "of it host", "of it transc.", "device calls", "ratio",
                                                                        "dev/one", "kernels of same_perm.hip, ms")
    lines = ["same-permutation prover, n_blinders = 4, runs alternating, median (min .. max) of %d runs after %d warm-up runs, ms per call over all items" % (a.runs, WARMUP), head]
    cases = []
    for ell, nb in SHAPES:
        for count in COUNTS:
            case = Case(ctx, ell, nb, count, points, rnd)
            cases.append(case)
            got = case.one_call()
            assert got == case.composed(), "the two routes disagree"
            case.proofs = got[0]
            ctx.set_profiling(True)
            ctx.reset_stats()
            case.one_call()
            ks = ctx.stat("k_same_perm_step")["ms"]
            ctx.set_profiling(False)
            lines.append("%5d %6d | %s | k_step %.4f" % (ell + nb, count, measure(case, case.one_call, case.composed, a.runs), ks))
    lines += ["", "same-permutation verifier on the prover's proofs, the same shapes and method (the extra relation joins the item's one MSM: three more points per row)", head]
    for case in cases:
        got = case.verify_one()
        assert got == case.verify_composed() and got[0] == [True] * case.count, "the two verifier routes disagree"
        ctx.set_profiling(True)
        ctx.reset_stats()
        case.verify_one()
        ks = [ctx.stat(k)["ms"] for k in ("k_same_perm_verify_step", "k_same_perm_weights")]
        ctx.set_profiling(False)
        lines.append("%5d %6d | %s | k_verify_step %.4f k_weights %.4f" % (case.n, case.count, measure(case, case.verify_one, case.verify_composed, a.runs), *ks))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
