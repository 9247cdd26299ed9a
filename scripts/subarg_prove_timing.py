"""What InnerProductProof::new / SameMultiscalarProof::new cost as ONE call each (cpx_ipa_prove, cpx_same_msm_prove) against the composed
route they replace.

    python scripts/subarg_prove_timing.py [--runs 20] [--parent-lib PATH] [--out FILE]

n = 256 (the 8 rounds of either argument at ell = 252), count = 1, 16 and 256 independent items, runs alternating, 3 warm-up runs, then
the median of `--runs` runs on the host clock:
  one call   the whole `new` of all items in cpx_ipa_prove / cpx_same_msm_prove on explicit draws: one synchronisation
  composed   what a caller did before, with calls every earlier build has, for all items at once: the blinder solve on the host,
             cpx_g1_msm_many for the B points, step 1 through cpx_transcript_*, the rewrite of the vectors by alpha on the host,
             cpx_g1_scale for H = beta crs_H (IPA), cpx_ipa_rounds / cpx_same_msm_rounds, the serialisation on the host: three (SameMSM:
             two) synchronisations.  With --parent-lib it runs on a context of THAT build of the library, loaded beside this one in the
             same process (the build of the parent commit: the route uses nothing newer); without it, on this build.
             The host's Fr arithmetic is Python integers here (a Rust caller's is some hundred times faster), so its share is reported on
             its own, as is the transcript's; "device calls" is the composed route without either.  The encodings of the statement points
             and of vec_T / vec_U that step 1 hashes are made beforehand: a caller has them.
Before anything is timed the two routes' proof bytes and end states are compared for every item: they must be equal.
The per-kernel times of k_subarg_blinders / k_subarg_prove_setup come from one profiled call per shape (Context.stat).
Points are multiples of the generator by seeded scalars.  A record, not a threshold: no test depends on a time.

    python scripts/subarg_prove_timing.py --layers-ab --parent-lib PATH [--runs 20] [--out FILE]

instead compares this build with the parent's call for call — the four provers, their _rng forms and the four verifiers at count = 1 and
64 — and says how far two contexts of the parent's build lie apart on the same calls (layers_ab below; profiles/subarg_layers.md).
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
from curdleproofs_amd.params import R, fr_from_wire, fr_to_wire   # noqa: E402
from curdleproofs_amd.transcript import Transcript   # noqa: E402

FR, AFF, JAC, ST = 32, 96, 144, 216
N, LOG_N = 256, 8
COUNTS = (1, 16, 256)
WARMUP = 3
SHAPES = {"IPA": dict(first=2, nvec=2, terms=4, order=(0, 2, 1, 3), step=b"ipa_step1", chal=(b"ipa_alpha", b"ipa_beta")),
          "SameMSM": dict(first=3, nvec=1, terms=6, order=range(6), step=b"same_msm_step1", chal=(b"same_msm_alpha",))}


def blinders(c, d, r, z):
    """generate_ipa_blinders (inner_product_argument.rs:42-82) on integers: r_d"""
    n = len(c)
    omega = (sum(a * b for a, b in zip(r, d)) + sum(a * b for a, b in zip(z, c))) % R
    delta = sum(a * b for a, b in zip(r, z)) % R
    inv_c = pow(c[n - 2], -1, R)
    last = (r[n - 2] * inv_c * omega - delta) * pow((-r[n - 2] * inv_c * c[n - 1] + r[n - 1]) % R, -1, R) % R
    return z + [-inv_c * (last * c[n - 1] + omega) % R, last]


class Case:
    def __init__(self, ctx, old, kind, count, points, rnd):
        self.ctx, self.old, self.kind, self.count = ctx, old, kind, count
        sh = self.sh = SHAPES[kind]
        ipa = kind == "IPA"
        rot = lambda k: (points[AFF * k:] + points[:AFF * k])
        take = lambda buf, each, k: (buf * (k * each // len(buf) + 1))[:k * each]
        one = params.fp_to_wire(1)
        self.fam = [take(rot(7 * f), AFF, count * N) for f in range(2 if ipa else 3)]
        stmt_aff = [take(rot(100 + 31 * k), AFF, count) for k in range(3)]
        self.stmt = [b"".join(a[AFF * i:AFF * (i + 1)] + one for i in range(count)) for a in stmt_aff]
        self.stmt_aff = stmt_aff
        self.wit_int = [[rnd.randrange(1, R) for _ in range(count * N)] for _ in range(sh["nvec"])]
        self.wit = [b"".join(fr_to_wire(x) for x in v) for v in self.wit_int]
        self.z_int = [rnd.randrange(1, R) for _ in range(count)]
        self.z = b"".join(fr_to_wire(x) for x in self.z_int)
        self.de = 2 * N - 2 if ipa else N
        self.draws_int = [rnd.randrange(1, R) for _ in range(count * self.de)]
        self.draws = b"".join(fr_to_wire(x) for x in self.draws_int)
        self.state0 = Transcript.new(b"subarg_prove_timing").state * count
        self.pb = 48 * (sh["first"] + sh["terms"] * LOG_N) + FR * sh["nvec"]
        # what step 1 hashes besides the B points, made beforehand
        self.stmt_comp = [ctx.normalize(s, compressed=True)[1] for s in self.stmt]
        if not ipa:
            jac = lambda aff: b"".join(aff[AFF * i:AFF * (i + 1)] + one for i in range(len(aff) // AFF))
            self.tu_comp = [ctx.normalize(jac(self.fam[f]), compressed=True)[1] for f in (1, 2)]
        # ---- marshalled once
        self.c_in = [cpx._in(b) for b in self.fam + self.stmt + ([self.z] if ipa else []) + self.wit + [self.draws]]
        self.states, self.proofs = cpx._out(ST * count), cpx._out(self.pb * count)
        self.status = (ctypes.c_int * count)()
        self.fn = ctx._L.cpx_ipa_prove if ipa else ctx._L.cpx_same_msm_prove
        nf = sh["first"]
        self.b_lens = (ctypes.c_uint32 * (count * nf))(*([N] * (count * nf)))
        self.b_bases = cpx._in(b"".join(self.fam[f][AFF * N * i:AFF * N * (i + 1)] for i in range(count) for f in range(nf)))
        self.b_out = cpx._out(48 * count * nf)
        self.o_fam = [cpx._in(b) for b in self.fam]
        self.o_h, self.o_hin = cpx._out(AFF * count), cpx._in(stmt_aff[0])
        self.o_comp, self.o_fin = cpx._out(count * LOG_N * sh["terms"] * 48), cpx._out(count * sh["nvec"] * FR)
        self.t_host = self.t_transcript = 0.0

    def one_call(self):
        ctypes.memmove(self.states, self.state0, ST * self.count)
        self.ctx._check(self.fn(self.ctx._h, self.count, N, *self.c_in, self.states, self.proofs, None, self.status))
        return bytes(self.proofs), bytes(self.states)

    def composed(self):
        sh, old, L, count, ipa = self.sh, self.old, self.old._L, self.count, self.kind == "IPA"
        nf = sh["first"]
        t0 = time.perf_counter()
        r = [self.draws_int[self.de * i:self.de * i + N] for i in range(count)]
        if ipa:
            rd = [blinders(self.wit_int[0][N * i:N * (i + 1)], self.wit_int[1][N * i:N * (i + 1)], r[i], self.draws_int[self.de * i + N:self.de * (i + 1)]) for i in range(count)]
            sc = b"".join(self.draws[FR * self.de * i:FR * (self.de * i + N)] + b"".join(fr_to_wire(x) for x in rd[i]) for i in range(count))
        else:
            sc = b"".join(self.draws[FR * N * i:FR * N * (i + 1)] * 3 for i in range(count))
        self.t_host += time.perf_counter() - t0
        old._check(L.cpx_g1_msm_many(old._h, count * nf, self.b_lens, self.b_bases, cpx._in(sc), None, self.b_out))
        t0 = time.perf_counter()
        first = bytes(self.b_out)
        states = [(ctypes.c_uint8 * ST).from_buffer_copy(self.state0[:ST]) for _ in range(count)]
        g = (ctypes.c_uint8 * FR)()
        chal = []
        step = sh["step"]
        msg = lambda st, m: L.cpx_transcript_append_message(st, step, len(step), m, len(m))
        for i, st in enumerate(states):
            if ipa:
                msg(st, self.stmt_comp[1][48 * i:48 * (i + 1)])
                msg(st, self.stmt_comp[2][48 * i:48 * (i + 1)])
                L.cpx_transcript_append_scalar(st, step, len(step), self.z[FR * i:FR * (i + 1)])
            else:
                for k in range(3):
                    msg(st, self.stmt_comp[k][48 * i:48 * (i + 1)])
                for f in range(2):
                    msg(st, N.to_bytes(8, "little") + self.tu_comp[f][48 * N * i:48 * N * (i + 1)])
            for b in range(nf):
                msg(st, first[48 * (nf * i + b):48 * (nf * i + b + 1)])
            row = []
            for label in sh["chal"]:
                L.cpx_transcript_challenge_scalar(st, label, len(label), g)
                row.append(bytes(g))
            chal.append(row)
        self.t_transcript += time.perf_counter() - t0
        t0 = time.perf_counter()
        alphas = [fr_from_wire(row[0]) for row in chal]
        vecs = []
        for v in range(sh["nvec"]):
            blind = rd if (ipa and v == 1) else r
            vecs.append(b"".join(fr_to_wire(blind[i][t] + alphas[i] * self.wit_int[v][N * i + t]) for i in range(count) for t in range(N)))
        self.t_host += time.perf_counter() - t0
        st_all = (ctypes.c_uint8 * (ST * count)).from_buffer_copy(b"".join(bytes(s) for s in states))
        if ipa:
            old._check(L.cpx_g1_scale(old._h, self.o_hin, cpx._in(b"".join(row[1] for row in chal)), FR, count, self.o_h))
            old._check(L.cpx_ipa_rounds(old._h, count, N, self.o_fam[0], self.o_fam[1], self.o_h, cpx._in(vecs[0]), cpx._in(vecs[1]), st_all, self.o_comp, None, self.o_fin, None))
        else:
            old._check(L.cpx_same_msm_rounds(old._h, count, N, *self.o_fam, cpx._in(vecs[0]), st_all, self.o_comp, None, self.o_fin, None))
        t0 = time.perf_counter()
        comp, fin, terms = bytes(self.o_comp), bytes(self.o_fin), sh["terms"]
        proofs = []
        for i in range(count):
            pt = lambda j, q: comp[48 * ((i * LOG_N + j) * terms + q):48 * ((i * LOG_N + j) * terms + q + 1)]
            fins = b"".join(fr_from_wire(fin[FR * (sh["nvec"] * i + v):FR * (sh["nvec"] * i + v + 1)]).to_bytes(32, "little") for v in range(sh["nvec"]))
            proofs.append(first[48 * nf * i:48 * nf * (i + 1)] + b"".join(pt(j, q) for q in sh["order"] for j in range(LOG_N)) + fins)
        self.t_host += time.perf_counter() - t0
        return b"".join(proofs), bytes(st_all)


def layer_calls(count, points, rnd, maker):
    """[(name, call(ctx))]: the eight sub-argument calls and the four _rng prover forms on `count` items of n = N (ell = 252, 4 blinders), on
    seeded inputs that every context gets alike; the verifiers read what `maker`'s provers made of them (the statements are not consistent,
    so the verdicts are rejections: the work is the same).  Every context draws from rng streams of its own."""
    import struct
    from curdleproofs_amd.rng import StdRng
    n, ell, nb = N, N - 4, 4
    one = params.fp_to_wire(1)
    pts = lambda k, shift: ((points[AFF * shift:] + points[:AFF * shift]) * (k * AFF // len(points) + 1))[:k * AFF]
    jac = lambda k, shift: b"".join(pts(k, shift)[AFF * i:AFF * (i + 1)] + one for i in range(k))
    frs = lambda k: b"".join(fr_to_wire(rnd.randrange(1, R)) for _ in range(k))
    states = Transcript.new(b"subarg_layers").state * count
    G, Gp, T, U = (pts(count * n, 7 * f) for f in range(4))
    Ge, He, g_sum, h_sum = pts(count * ell, 3), pts(count * nb, 11), pts(count, 301), pts(count, 302)
    P = [jac(count, 100 + 31 * k) for k in range(3)]
    z, c, d = frs(count), frs(count * n), frs(count * n)
    res, b, rb, va, ra, rm = frs(count), frs(count * ell), frs(count * nb), frs(count * ell), frs(count * nb), frs(count * nb)
    perm = b"".join(struct.pack("<%dI" % ell, *rnd.sample(range(ell), ell)) for _ in range(count))
    draws = {"ipa": frs(count * (2 * n - 2)), "same_msm": frs(count * n), "gprod": frs(count * (nb + 2 * n - 2))}
    draws["same_perm"] = draws["gprod"]
    prove = {"ipa": lambda cx, **kw: cx.ipa_prove(n, G, Gp, *P, z, c, d, states, **kw),
             "same_msm": lambda cx, **kw: cx.same_msm_prove(n, G, T, U, *P, c, states, **kw),
             "gprod": lambda cx, **kw: cx.gprod_prove(ell, Ge, He, P[0], P[1], res, b, rb, states, **kw),
             "same_perm": lambda cx, **kw: cx.same_perm_prove(ell, Ge, He, P[0], P[1], P[2], va, perm, ra, rm, states, **kw)}
    proofs = {k: b"".join(prove[k](maker, rand=draws[k])["proofs"]) for k in prove}
    f2, f3 = frs(2 * count), frs(3 * count)
    verify = {"ipa": lambda cx: cx.ipa_verify(n, G, *P, z, d, proofs["ipa"], f2, states),
              "same_msm": lambda cx: cx.same_msm_verify(n, G, T, U, *P, proofs["same_msm"], f3, states),
              "gprod": lambda cx: cx.gprod_verify(ell, Ge, He, P[0], g_sum, h_sum, P[1], res, proofs["gprod"], f2, states),
              "same_perm": lambda cx: cx.same_perm_verify(ell, Ge, He, P[0], g_sum, h_sum, P[1], P[2], va, proofs["same_perm"], f3, states)}
    streams = {}
    own = lambda cx: streams.setdefault(id(cx), [StdRng(rnd.randbytes(32) + bytes(8)) for _ in range(count)])
    calls = []
    for k in prove:
        calls.append((k + "_prove", lambda cx, k=k: prove[k](cx, rand=draws[k])))
        calls.append((k + "_prove_rng", lambda cx, k=k: prove[k](cx, rngs=own(cx))))
        calls.append((k + "_verify", verify[k]))
    return calls


def layers_ab(a):
    """--layers-ab: host time per call of this build against the parent's (--parent-lib), call for call, in one process.  Three contexts — the
    parent's build, a second context of the parent's build, this build — take every call in turn, runs alternating; the medians of the two
    parent contexts against each other (A/A) say how far two medians of the same code lie apart, the largest such spread over all shapes is
    the margin this build's median is held to against the parent's (A/B)."""
    ctxs = [("parent", cpx.Context(0, lib=a.parent_lib)), ("parent again", cpx.Context(0, lib=a.parent_lib)), ("this build", cpx.Context(0))]
    rnd = random.Random(20261021)
    points = ctxs[0][1].generator_mul(params.random_fr_wire(rnd, 2048))
    lines = ["sub-argument calls at n = %d (ell = %d, 4 blinders), ms per call over all items on the host clock, median of %d runs after %d warm-up runs," % (N, N - 4, a.runs, WARMUP),
             "the three contexts in turn within every run",
             "%-20s %6s | %10s %12s %8s | %10s %8s" % ("call", "count", "parent", "parent again", "A/A", "this build", "A/B")]
    spread, worst = 0.0, 0.0
    for count in (1, 64):
        for name, call in layer_calls(count, points, rnd, ctxs[0][1]):
            times = [[] for _ in ctxs]
            for run in range(WARMUP + a.runs):
                for k in range(len(ctxs)):
                    at = (k + run) % len(ctxs)   # the order within a run rotates
                    t0 = time.perf_counter()
                    call(ctxs[at][1])
                    if run >= WARMUP:
                        times[at].append(time.perf_counter() - t0)
            p, p2, t = (1e3 * statistics.median(v) for v in times)
            spread, worst = max(spread, abs(p2 / p - 1)), max(worst, t / p - 1)
            lines.append("%-20s %6d | %10.3f %12.3f %+7.2f%% | %10.3f %+7.2f%%" % (name, count, p, p2, 100 * (p2 / p - 1), t, 100 * (t / p - 1)))
    lines.append("margin (the largest A/A spread): %.2f%%; this build's largest excess over the parent: %+.2f%%: %s" % (100 * spread, 100 * worst,
                                                                                                                  "within the margin" if worst <= spread else "OUTSIDE the margin"))
    for _, cx in ctxs:
        cx.close()
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--parent-lib", help="libcpx.so of the parent commit: the composed route runs on a context of that build")
    ap.add_argument("--layers-ab", action="store_true", help="instead: all eight sub-argument calls and the _rng prover forms, this build against --parent-lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.layers_ab:
        if not a.parent_lib:
            ap.error("--layers-ab needs --parent-lib")
        text = layers_ab(a)
        print(text)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(text + "\n")
        return 0
    ctx = cpx.Context(0)
    old = cpx.Context(0, lib=a.parent_lib) if a.parent_lib else ctx
    rnd = random.Random(20261021)
    points = ctx.generator_mul(params.random_fr_wire(rnd, 2048))
    lines = ["sub-argument provers at n = %d (%d rounds), runs alternating, median of %d runs after %d warm-up runs, ms per call over all items" % (N, LOG_N, a.runs, WARMUP),
             "composed route on %s" % ("a context of the build given as --parent-lib, in the same process" if a.parent_lib else "this build"),
             "%-8s %6s | %10s %10s | %10s %12s %14s %12s | %8s %8s | %16s %20s" % ("prover", "count", "one call", "per item", "composed", "of it host", "of it transcr.", "device calls",
                                                                             "ratio", "dev/one", "k_subarg_blinders", "k_subarg_prove_setup")]
    for kind in SHAPES:
        for count in COUNTS:
            case = Case(ctx, old, kind, count, points, rnd)
            assert case.one_call() == case.composed(), "the two routes disagree"
            assert all(s == cpx.CPX_OK for s in case.status)
            ctx.set_profiling(True)
            ctx.reset_stats()
            case.one_call()
            kb, ks = ctx.stat("k_subarg_blinders")["ms"], ctx.stat("k_subarg_prove_setup")["ms"]
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
                    acc.append(time.perf_counter() - t0)
            one, comp = 1e3 * statistics.median(t_one), 1e3 * statistics.median(t_comp)
            host, tr = 1e3 * case.t_host / a.runs, 1e3 * case.t_transcript / a.runs
            lines.append("%-8s %6d | %10.3f %10.4f | %10.3f %12.3f %14.3f %12.3f | %8.2f %8.2f | %16.4f %20.4f" % (kind, count, one, one / count, comp, host, tr, comp - host - tr,
                                                                                                   comp / one, (comp - host - tr) / one, kb, ks))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    if old is not ctx:
        old.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
