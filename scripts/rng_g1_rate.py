"""What drawing G1 points on the device costs: cpx_rng_g1 (G1Projective::rand from ChaCha12 states; kernels k_rng_g1_scan, k_rng_g1_sqrt,
k_rng_g1_select, k_clear_cofactor) at a few shapes, one context.

    python scripts/rng_g1_rate.py [--shapes 1x259,1x1027,1024x504,8192x504] [--runs 5] [--out FILE.md]

For every shape count x n_each: one stream per item split off one parent; the figures are medians of --runs calls on the host clock after
one warm-up call, at the C-ABI with the buffers allocated beforehand (affine output only).  Beside them: every kernel's own time from the
library's kernel statistics (a profiled call of its own), how many rounds the call took (read-only option rng_g1_last_rounds), and — for
context — the points per second ONE host thread of the CPU oracle (tests/oracle_lib.py, test infrastructure) draws at 1 x 259 on the same
box (n/a where the oracle is not built).
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import curdleproofs_amd as cpx   # noqa: E402
from curdleproofs_amd.rng import StdRng   # noqa: E402

KERNELS = ("k_rng_g1_scan", "k_rng_g1_sqrt", "k_rng_g1_select", "k_clear_cofactor")


def oracle_rate(n):
    try:
        from tests.oracle_lib import Oracle
        o = Oracle().rng(1)
        o.g1_affine(8)
        t0 = time.perf_counter()
        o.g1_affine(n)
        return n / (time.perf_counter() - t0)
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x259,1x1027,1024x504,8192x504")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = cpx.Context(0)
    L, h = ctx._L, ctx._h
    say("# rng_g1_rate: cpx_rng_g1, runs = %d (median, host clock), rng_g1_round_cap = %d" % (a.runs, ctx.get_option("rng_g1_round_cap")))
    say("")
    say("| streams x points | call ms | points/s | rounds | " + " | ".join("`%s` ms" % k for k in KERNELS) + " | min - max ms |")
    say("|---|---|---|---|" + "---|" * len(KERNELS) + "---|")
    for shape in a.shapes.split(","):
        count, n_each = (int(x) for x in shape.split("x"))
        start = b"".join(c.state for c in StdRng.seed_from_u64(1).split(count))
        st = (ctypes.c_uint8 * len(start))()
        out = (ctypes.c_uint8 * (96 * count * n_each))()

        def call():
            ctypes.memmove(st, start, len(start))
            ctx._check(L.cpx_rng_g1(h, count, st, n_each, out, None))

        call()
        ts = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        rounds = ctx.get_option("rng_g1_last_rounds")
        ctx.set_profiling(True)
        ctx.reset_stats()
        call()
        ks = [ctx.stat(k)["ms"] for k in KERNELS]
        ctx.set_profiling(False)
        t = statistics.median(ts)
        say("| %d x %d | %.2f | %.0f | %d | %s | %.2f - %.2f |" % (count, n_each, 1e3 * t, count * n_each / t, rounds, " | ".join("%.3f" % k for k in ks), 1e3 * min(ts), 1e3 * max(ts)))
    say("")
    r = oracle_rate(259)
    say("CPU oracle, one thread, 1 x 259: %s points/s" % ("n/a" if r is None else "%.0f" % r))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
