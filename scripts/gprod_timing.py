"""What GrandProductProof::new and ::verify cost as ONE call each (cpx_gprod_prove, cpx_gprod_verify) against the composed routes they
replace, on the same build.

    python scripts/gprod_timing.py [--runs 20] [--out FILE]

n = 128 and n = 256 with n_blinders = 4 (ell = 124 and 252), count = 1, 16 and 256 independent items, runs alternating, 3 warm-up runs,
then the median of `--runs` runs on the host clock with the smallest and the largest run beside it:
  one call   the whole `new` of all items in cpx_gprod_prove on explicit draws: one synchronisation
  composed   what a caller of the stand-alone route does today, item by item for the grand-product layer: the prefix products, r_p, the
             powers of beta, vec_d and inner_prod on the host, gprod_step1 / gprod_step2 through cpx_transcript_*, Context.msm for C,
             Context.scale for G' = u o (G | H), Context.msm for D (over G | H and B, B with a unit scalar); then ONE Context.ipa_prove
             over all items on the 2 n uploaded bases.
             The host's Fr arithmetic is Python integers here (a Rust caller's is some hundred times faster), so its share is reported
             on its own, as is the transcript's; "device calls" is the composed route without either.
Before anything is timed the two routes' proof bytes and end states are compared for every item: they must be equal.
The per-kernel times of k_gprod_products / k_gprod_setup / k_gprod_rdu come from one profiled call per shape (Context.stat).
Points are multiples of the generator by seeded scalars.  A record, not a threshold: no test depends on a time.
The verifier likewise, on the proofs the prover made:
  one call   cpx_gprod_verify over all items: one synchronisation
  composed   per item gprod_step1 / gprod_step2 through cpx_transcript_*, vec_u and inner_prod on the host, Context.msm for
             D = B - beta^-1 crs_G_sum + alpha crs_H_sum; then ONE Context.ipa_verify over all items.
Both must give the same verdicts (all accepted) and end states.
"""
import argparse
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import curdleproofs_amd as cpx   # noqa: E402
from curdleproofs_amd import params   # noqa: E402
from curdleproofs_amd.params import R, fr_from_wire, fr_to_wire   # noqa: E402
from curdleproofs_amd.transcript import Transcript   # noqa: E402

FR, AFF, JAC, ST = 32, 96, 144, 216
SHAPES = ((124, 4), (252, 4))
COUNTS = (1, 16, 256)
WARMUP = 3


class Case:
    def __init__(self, ctx, ell, nb, count, points, rnd):
        self.ctx, self.ell, self.nb, self.count = ctx, ell, nb, count
        n = self.n = ell + nb
        self.L = n.bit_length() - 1
        rot = lambda k: (points[AFF * k:] + points[:AFF * k])
        take = lambda buf, each, k: (buf * (k * each // len(buf) + 1))[:k * each]
        one = params.fp_to_wire(1)
        jac = lambda aff: b"".join(aff[AFF * i:AFF * (i + 1)] + one for i in range(len(aff) // AFF))
        self.G, self.H = take(rot(0), AFF, count * ell), take(rot(900), AFF, count * nb)
        self.U_aff = take(rot(100), AFF, count)
        self.U = jac(self.U_aff)
        self.b_int = [rnd.randrange(1, R) for _ in range(count * ell)]
        self.rb_int = [rnd.randrange(1, R) for _ in range(count * nb)]
        wire = lambda v: b"".join(fr_to_wire(x) for x in v)
        # a statement the witness satisfies (grand_product_argument.rs:292-298): gprod_result = prod b, B = <b, G> + <r_b, H>
        self.res_int = []
        for i in range(count):
            prod = 1
            for x in self.b_int[ell * i:ell * (i + 1)]:
                prod = prod * x % R
            self.res_int.append(prod)
        self.B_aff = b"".join(ctx.normalize(ctx.msm(self.G[AFF * ell * i:AFF * ell * (i + 1)] + self.H[AFF * nb * i:AFF * nb * (i + 1)],
                                                    wire(self.b_int[ell * i:ell * (i + 1)] + self.rb_int[nb * i:nb * (i + 1)]))) for i in range(count))
        self.B = jac(self.B_aff)
        self.b, self.rb, self.res = wire(self.b_int), wire(self.rb_int), wire(self.res_int)
        self.de = nb + 2 * n - 2
        self.draws_int = [rnd.randrange(1, R) for _ in range(count * self.de)]
        self.draws = wire(self.draws_int)
        self.state0 = Transcript.new(b"gprod_timing").state
        self.B_comp = ctx.normalize(self.B, compressed=True)[1]           # what step 1 hashes, made beforehand: a caller has it
        ones = fr_to_wire(1)
        sums = lambda pts, each: b"".join(ctx.normalize(ctx.msm(pts[AFF * each * i:AFF * each * (i + 1)], ones * each)) if each else bytes(AFF) for i in range(count))
        self.g_sum, self.h_sum = sums(self.G, ell), sums(self.H, nb)       # the CRS sums: a verifier has them
        self.vrand = wire([rnd.randrange(1, R) for _ in range(2 * count)])
        self.proofs = None
        self.v_host = self.v_transcript = 0.0
        self.t_host = self.t_transcript = 0.0

    def one_call(self):
        out = self.ctx.gprod_prove(self.ell, self.G, self.H, self.U, self.B, self.res, self.b, self.rb, self.state0 * self.count, rand=self.draws)
        assert all(s is True for s in out["status"])
        return b"".join(out["proofs"]), out["states"]

    def composed(self):
        ctx, ell, nb, n, count = self.ctx, self.ell, self.nb, self.n, self.count
        wire = lambda v: b"".join(fr_to_wire(x % R) for x in v)
        one = params.fp_to_wire(1)
        Gs, Gps, Cs, Ds, zs, cs, ds, states, heads, ipa_draws = [], [], [], [], [], [], [], [], [], []
        for i in range(count):
            t0 = time.perf_counter()
            b, rb = self.b_int[ell * i:ell * (i + 1)], self.rb_int[nb * i:nb * (i + 1)]
            dr = self.draws_int[self.de * i:self.de * (i + 1)]
            cbl = dr[:nb]
            c = [1]
            for x in b[:-1]:
                c.append(c[-1] * x % R)
            c += cbl
            self.t_host += time.perf_counter() - t0
            GH = self.G[AFF * ell * i:AFF * ell * (i + 1)] + self.H[AFF * nb * i:AFF * nb * (i + 1)]
            C = ctx.msm(GH, wire(c))
            C_comp = ctx.normalize(C, compressed=True)[1]
            t0 = time.perf_counter()
            t = Transcript.from_state(self.state0)
            t.append_message(b"gprod_step1", self.B_comp[48 * i:48 * (i + 1)])
            t.append_scalar(b"gprod_step1", self.res[FR * i:FR * (i + 1)])
            alpha = fr_from_wire(t.challenge_scalar(b"gprod_alpha"))
            self.t_transcript += time.perf_counter() - t0
            t0 = time.perf_counter()
            r_p = sum((x + alpha) * y for x, y in zip(rb, cbl)) % R
            self.t_host += time.perf_counter() - t0
            t0 = time.perf_counter()
            t.append_message(b"gprod_step2", C_comp)
            t.append_scalar(b"gprod_step2", fr_to_wire(r_p))
            beta = fr_from_wire(t.challenge_scalar(b"gprod_beta"))
            self.t_transcript += time.perf_counter() - t0
            t0 = time.perf_counter()
            bi = pow(beta, -1, R)
            pw, ipw, u, d = 1, bi, [], []
            for x in b:
                d.append((x * pw * beta - pw) % R)
                u.append(ipw)
                pw, ipw = pw * beta % R, ipw * bi % R
            u += [ipw] * nb                                                # pw = beta^ell, ipw = beta^-(ell+1)
            d += [pw * beta * (x + alpha) % R for x in rb]
            inner = (r_p * pw * beta + self.res_int[i] * pw - 1) % R
            dsc = [-bi] * ell + [alpha] * nb + [1]
            self.t_host += time.perf_counter() - t0
            Gp = ctx.scale(GH, wire(u))
            D = ctx.msm(GH + self.B_aff[AFF * i:AFF * (i + 1)], wire(dsc))
            Gs.append(GH), Gps.append(Gp), Cs.append(C), Ds.append(D), zs.append(fr_to_wire(inner)), cs.append(wire(c)), ds.append(wire(d))
            states.append(t.state)
            heads.append(C_comp + r_p.to_bytes(32, "little"))
            ipa_draws.append(self.draws[FR * (self.de * i + nb):FR * self.de * (i + 1)])
        cat = b"".join
        out = ctx.ipa_prove(n, cat(Gs), cat(Gps), self.U, cat(Cs), cat(Ds), cat(zs), cat(cs), cat(ds), cat(states), rand=cat(ipa_draws))
        return cat(h + p for h, p in zip(heads, out["proofs"])), out["states"]


def verify_one(case):
    out = case.ctx.gprod_verify(case.ell, case.G, case.H, case.U, case.g_sum, case.h_sum, case.B, case.res, case.proofs, case.vrand, case.state0 * case.count)
    return out["verdicts"], out["states"]


def verify_composed(case):
    ctx, ell, nb, n, count = case.ctx, case.ell, case.nb, case.n, case.count
    pb = len(case.proofs) // count
    wire = lambda v: b"".join(fr_to_wire(x % R) for x in v)
    one = params.fp_to_wire(1)
    Gs, Cs, Ds, zs, us, states, inner = [], [], [], [], [], [], []
    for i in range(count):
        proof = case.proofs[pb * i:pb * (i + 1)]
        t0 = time.perf_counter()
        t = Transcript.from_state(case.state0)
        t.append_message(b"gprod_step1", case.B_comp[48 * i:48 * (i + 1)])
        t.append_scalar(b"gprod_step1", case.res[FR * i:FR * (i + 1)])
        alpha = fr_from_wire(t.challenge_scalar(b"gprod_alpha"))
        r_p = int.from_bytes(proof[48:80], "little")
        t.append_message(b"gprod_step2", proof[:48])
        t.append_scalar(b"gprod_step2", fr_to_wire(r_p))
        beta = fr_from_wire(t.challenge_scalar(b"gprod_beta"))
        case.v_transcript += time.perf_counter() - t0
        t0 = time.perf_counter()
        bi = pow(beta, -1, R)
        u, ipw = [], bi
        for _ in range(ell):
            u.append(ipw)
            ipw = ipw * bi % R
        u += [ipw] * nb
        z = (r_p * pow(beta, ell + 1, R) + case.res_int[i] * pow(beta, ell, R) - 1) % R
        case.v_host += time.perf_counter() - t0
        D = ctx.msm(case.g_sum[AFF * i:AFF * (i + 1)] + case.h_sum[AFF * i:AFF * (i + 1)] + case.B_aff[AFF * i:AFF * (i + 1)], wire([-bi, alpha, 1]))
        Gs.append(case.G[AFF * ell * i:AFF * ell * (i + 1)] + case.H[AFF * nb * i:AFF * nb * (i + 1)])
        Cs.append(ctx.decompress(proof[:48]) + one), Ds.append(D), zs.append(fr_to_wire(z)), us.append(wire(u)), states.append(t.state), inner.append(proof[80:])
    cat = b"".join
    out = ctx.ipa_verify(n, cat(Gs), case.U, cat(Cs), cat(Ds), cat(zs), cat(us), cat(inner), case.vrand, cat(states))
    return out["verdicts"], out["states"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = cpx.Context(0)
    rnd = random.Random(20261021)
    points = ctx.generator_mul(params.random_fr_wire(rnd, 2048))
    lines = ["grand-product prover, n_blinders = 4, runs alternating, median (min .. max) of %d runs after %d warm-up runs, ms per call over all items" % (a.runs, WARMUP),
             "%5s %6s | %28s %10s | %30s %10s %12s %12s | %8s %8s | %10s %10s %10s" % ("n", "count", "one call", "per item", "composed", "of it host", "of it transc.", "device calls",
                                                                                   "ratio", "dev/one", "k_products", "k_setup", "k_rdu")]
    for ell, nb in SHAPES:
        for count in COUNTS:
            case = Case(ctx, ell, nb, count, points, rnd)
            assert case.one_call() == case.composed(), "the two routes disagree"
            ctx.set_profiling(True)
            ctx.reset_stats()
            case.one_call()
            ks = [ctx.stat(k)["ms"] for k in ("k_gprod_products", "k_gprod_setup", "k_gprod_rdu")]
            ctx.set_profiling(False)
            for _ in range(WARMUP):
                case.one_call()
                case.composed()
            case.t_host = case.t_transcript = 0.0
            t_one, t_comp = [], []
            for _ in range(a.runs):
                for fn, acc in ((case.one_call, t_one), (case.composed, t_comp)):
                    t0 = time.perf_counter()
                    fn()
                    acc.append(1e3 * (time.perf_counter() - t0))
            one, comp = statistics.median(t_one), statistics.median(t_comp)
            host, tr = 1e3 * case.t_host / a.runs, 1e3 * case.t_transcript / a.runs
            lines.append("%5d %6d | %9.3f (%7.3f .. %7.3f) %10.4f | %10.3f (%8.3f .. %8.3f) %10.3f %12.3f %12.3f | %8.2f %8.2f | %10.4f %10.4f %10.4f" % (
                ell + nb, count, one, min(t_one), max(t_one), one / count, comp, min(t_comp), max(t_comp), host, tr, comp - host - tr, comp / one, (comp - host - tr) / one, *ks))
    lines += ["", "grand-product verifier on the prover's proofs, the same shapes and method",
              "%5s %6s | %28s %10s | %30s %10s %12s %12s | %8s %8s | %10s" % ("n", "count", "one call", "per item", "composed", "of it host", "of it transc.", "device calls", "ratio",
                                                                            "dev/one", "k_steps")]
    for ell, nb in SHAPES:
        for count in COUNTS:
            case = Case(ctx, ell, nb, count, points, rnd)
            case.proofs = case.one_call()[0]
            got = verify_one(case)
            assert got == verify_composed(case) and got[0] == [True] * count, "the two verifier routes disagree"
            ctx.set_profiling(True)
            ctx.reset_stats()
            verify_one(case)
            ks = ctx.stat("k_gprod_verify_steps")["ms"]
            ctx.set_profiling(False)
            for _ in range(WARMUP):
                verify_one(case)
                verify_composed(case)
            case.v_host = case.v_transcript = 0.0
            t_one, t_comp = [], []
            for _ in range(a.runs):
                for fn, acc in ((verify_one, t_one), (verify_composed, t_comp)):
                    t0 = time.perf_counter()
                    fn(case)
                    acc.append(1e3 * (time.perf_counter() - t0))
            one, comp = statistics.median(t_one), statistics.median(t_comp)
            host, tr = 1e3 * case.v_host / a.runs, 1e3 * case.v_transcript / a.runs
            lines.append("%5d %6d | %9.3f (%7.3f .. %7.3f) %10.4f | %10.3f (%8.3f .. %8.3f) %10.3f %12.3f %12.3f | %8.2f %8.2f | %10.4f" % (
                ell + nb, count, one, min(t_one), max(t_one), one / count, comp, min(t_comp), max(t_comp), host, tr, comp - host - tr, comp / one, (comp - host - tr) / one, ks))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
