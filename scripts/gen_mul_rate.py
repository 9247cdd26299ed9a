"""Rate of cpx_whisk_trackers_from_k_r (the generator's fixed-base table, genmul.hip) against the route the library offered before it for
the same outputs, in one process and on one context.

    python scripts/gen_mul_rate.py [--counts 65536,1048576] [--runs 5] [--out FILE]

Both routes take the same seeded (k, r) pairs (non-zero with overwhelming probability) and write the same `count` serialized trackers
r G || k r G (96 bytes each); the bytes are compared.  The earlier route is cpx_g1_scale of G with per-element scalars r, a second cpx_g1_scale of those points by k, and one
cpx_g1_normalize with compression over the 2 count points (the host only interleaves the two point arrays and appends Z = 1, with numpy).
Per count: one warm-up of each route, then `--runs` timed repetitions with the two routes alternating, host clock around calls that end
in a stream synchronisation; the medians are reported.  Buffers are marshalled beforehand.  The one-off table build is the k_gen_table
kernel time of a fresh context's first call (profiling on), and that call's wall time beside an identical second call.  Prints plain
lines; exit status 1 if the two routes disagree.
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import curdleproofs_amd as cpx   # noqa: E402
from curdleproofs_amd import params   # noqa: E402


def table_build(lines):
    c = cpx.Context(0)
    try:
        c.set_profiling(True)
        k = params.random_fr_wire(random.Random(1), 1)
        t0 = time.perf_counter()
        c.generator_mul(k)
        t1 = time.perf_counter()
        c.generator_mul(k)
        t2 = time.perf_counter()
        lines.append("table build: k_gen_table %.3f ms (kernel, once per context); first call %.2f ms wall, second call %.2f ms wall"
                     % (c.stat("k_gen_table")["ms"], 1e3 * (t1 - t0), 1e3 * (t2 - t1)))
    finally:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="65536,1048576")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    counts = [int(c) for c in a.counts.split(",")]
    if a.runs < 5:
        ap.error("--runs: at least 5 repetitions")
    lines = []
    table_build(lines)
    ctx = cpx.Context(0)
    L, h = ctx._L, ctx._h
    nmax = max(counts)
    # seeded wire scalars: 32 random bytes with the top two bits cleared are limbs below r, the Montgomery form of some field element
    limbs = np.random.RandomState(20261017).randint(0, 256, size=(2, nmax, 32), dtype=np.uint8)
    limbs[:, :, 31] &= 0x3f
    ks, rs = limbs[0].tobytes(), limbs[1].tobytes()
    one = np.frombuffer(params.fp_to_wire(1), dtype=np.uint8)
    ok = True
    for n in counts:
        k, r = cpx._in(ks[:32 * n]), cpx._in(rs[:32 * n])
        gens = cpx._in(params.g1_generator_wire() * n)
        r_g, k_r_g, jac = cpx._out(96 * n), cpx._out(96 * n), cpx._out(144 * 2 * n)
        old_out, new_out = cpx._out(96 * n), cpx._out(96 * n)
        jv = np.frombuffer(jac, dtype=np.uint8).reshape(n, 2, 144)
        jv[:, :, 96:] = one                                        # Z = 1 (random non-zero scalars: no identity among the points)

        def old_route():
            ctx._check(L.cpx_g1_scale(h, gens, r, 32, n, r_g))
            ctx._check(L.cpx_g1_scale(h, r_g, k, 32, n, k_r_g))
            jv[:, 0, :96] = np.frombuffer(r_g, dtype=np.uint8).reshape(n, 96)
            jv[:, 1, :96] = np.frombuffer(k_r_g, dtype=np.uint8).reshape(n, 96)
            ctx._check(L.cpx_g1_normalize(h, jac, 2 * n, None, old_out))

        def new_route():
            ctx._check(L.cpx_whisk_trackers_from_k_r(h, n, k, r, new_out, None))

        old_route()
        new_route()
        t_old, t_new = [], []
        for _ in range(a.runs):
            for fn, acc in ((old_route, t_old), (new_route, t_new)):
                t0 = time.perf_counter()
                fn()
                acc.append(time.perf_counter() - t0)
        same = bytes(old_out) == bytes(new_out)
        ok &= same
        m_old, m_new = statistics.median(t_old), statistics.median(t_new)
        lines.append("count %d, %d alternating runs: cpx_g1_scale x2 + cpx_g1_normalize %.1f ms (%.0f trackers/s, min %.1f max %.1f ms); "
                     "cpx_whisk_trackers_from_k_r %.1f ms (%.0f trackers/s, min %.1f max %.1f ms); ratio %.2f; same bytes: %s"
                     % (n, a.runs, 1e3 * m_old, n / m_old, 1e3 * min(t_old), 1e3 * max(t_old), 1e3 * m_new, n / m_new, 1e3 * min(t_new), 1e3 * max(t_new),
                        m_old / m_new, same))
        ctx.set_profiling(True)
        ctx.reset_stats()
        new_route()
        g, c = ctx.stat("k_gen_mul"), ctx.stat("k_compress")
        ctx.reset_stats()
        old_route()
        s = ctx.stat("k_smul")
        ctx.set_profiling(False)
        lines.append("count %d, kernel times: k_gen_mul %.2f ms (%d points), k_compress %.2f ms; k_smul %.2f ms in %d launches (%d points)"
                     % (n, g["ms"], g["units"], c["ms"], s["ms"], s["launches"], s["units"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
