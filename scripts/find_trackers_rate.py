"""Rate of cpx_whisk_find_trackers (find.hip) against the route the library offered before it, the crossover between its two paths, and
the kernel times of its table path — in one process.

    python scripts/find_trackers_rate.py [--trackers 8192] [--runs 5] [--out profiles/find_trackers.md]

Inputs are seeded: `--trackers` trackers r_i G || k r_i G made with cpx_whisk_trackers_from_k_r from seeded scalars, tracker i with key
i mod 1024 of a seeded key set, so every run of n_keys keys (the first n_keys of the set) has owners to find.  Buffers are marshalled
beforehand.  Three parts:

 1. against the earlier route, n_keys in {1, 64, 1024}: that route decodes the 2 n points with one cpx_g1_decompress, then per key runs one
    cpx_g1_scale with a shared scalar over the decoded r_G and compares the bytes with the decoded k_r_G in numpy.  Decoding is inside both
    routes.  The owners of both are compared with each other and with the planted ones.
 2. both paths of the new call forced (find_table_min_keys = 1 / 2^20 + 1) at n_keys in {16, 32, 64, 128, 256}: the smallest measured power
    of two at which the table path's median is below the ladder's is what the default of find_table_min_keys should be.
 3. the kernel times of the table path at n_keys = 1024 with profiling on, and the scan's field products per second (32 mixed additions of
    10 products per pair: an upper bound, a zero digit is skipped) beside cpx_bench_fpmul's figure from the same run.

Per shape and route: one warm-up, then `--runs` (at least 5) timed repetitions with the routes alternating, host clock around calls that
end in a stream synchronisation; medians and min - max are reported.  Exit status 1 if any two routes disagree.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import curdleproofs_amd as cpx   # noqa: E402

KEY_SET = 1024
NEVER_TABLE = (1 << 20) + 1
NO_OWNER = 0xffffffff


def timed(routes, runs):
    """routes: [(name, fn)]; one warm-up each, then `runs` rounds with the routes alternating.  Returns {name: [seconds]}"""
    for _, fn in routes:
        fn()
    t = {name: [] for name, _ in routes}
    for _ in range(runs):
        for name, fn in routes:
            t0 = time.perf_counter()
            fn()
            t[name].append(time.perf_counter() - t0)
    return t


def ms(ts):
    return "%.2f (%.2f - %.2f)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trackers", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: at least 5 repetitions")
    n = a.trackers
    ctx = cpx.Context(0)
    L, h = ctx._L, ctx._h
    # seeded wire scalars: 32 random bytes with the top two bits cleared are limbs below r, the Montgomery form of some field element
    limbs = np.random.RandomState(20261019).randint(0, 256, size=(KEY_SET + n, 32), dtype=np.uint8)
    limbs[:, 31] &= 0x3f
    keys_np, rs_np = limbs[:KEY_SET], limbs[KEY_SET:]
    planted = np.arange(n) % KEY_SET
    trk = cpx._out(96 * n)
    ctx._check(L.cpx_whisk_trackers_from_k_r(h, n, cpx._in(keys_np[planted].tobytes()), cpx._in(rs_np.tobytes()), trk, None))
    trackers = cpx._in(bytes(trk))
    tv = np.frombuffer(trackers, dtype=np.uint8).reshape(n, 2, 48)
    halves = cpx._in(np.ascontiguousarray(tv.transpose(1, 0, 2)).tobytes())      # the earlier route's input: all r_G, then all k_r_G
    owner, status = (ctypes.c_uint32 * n)(), (ctypes.c_int * n)()
    dec, prod = cpx._out(96 * 2 * n), cpx._out(96 * n)
    dec_v = np.frombuffer(dec, dtype=np.uint8).reshape(2, n, 96)
    prod_v = np.frombuffer(prod, dtype=np.uint8).reshape(n, 96)
    r_g = (ctypes.c_uint8 * (96 * n)).from_buffer(dec)                            # the decoded r_G, in place
    ok = True
    out = ["# cpx_whisk_find_trackers: rates, crossover, kernel times", "",
           "`python scripts/find_trackers_rate.py` on one MI355X, one process, %d seeded trackers, tracker i made with key i mod %d of a seeded set;"
           % (n, KEY_SET),
           "a call with n_keys keys takes the first n_keys of the set.  Host clock around calls that end in a stream synchronisation, buffers",
           "marshalled beforehand, one warm-up per route, then %d timed repetitions with the routes alternating.  ms: median (min - max)." % a.runs, ""]

    def new_call(nk, keys):
        def f():
            ctx._check(L.cpx_whisk_find_trackers(h, n, trackers, nk, keys, owner, status))
        return f

    def old_call(nk, keys_bytes, result):
        key_bufs = [cpx._in(keys_bytes[32 * j:32 * (j + 1)]) for j in range(nk)]

        def f():
            ctx._check(L.cpx_g1_decompress(h, halves, 2 * n, dec, 1))
            own = np.full(n, NO_OWNER, dtype=np.uint32)
            for j in reversed(range(nk)):                                        # (descending: the smallest matching index is written last)
                ctx._check(L.cpx_g1_scale(h, r_g, key_bufs[j], 0, n, prod))
                own[(prod_v == dec_v[1]).all(axis=1)] = j
            result[:] = own
        return f

    def want(nk):
        return np.where(planted < nk, planted, NO_OWNER).astype(np.uint32)

    # ---- 1. against the earlier route ----
    out += ["## 1. Against one `cpx_g1_scale` per key and a byte compare on the host", "",
            "| trackers | keys | earlier route ms | `cpx_whisk_find_trackers` ms (default options) | path | earlier / new | same owners |", "|---|---|---|---|---|---|---|"]
    for nk in (1, 64, 1024):
        kb = keys_np[:nk].tobytes()
        keys = cpx._in(kb)
        old_own = np.zeros(n, dtype=np.uint32)
        t = timed([("old", old_call(nk, kb, old_own)), ("new", new_call(nk, keys))], a.runs)
        new_own = np.frombuffer(owner, dtype=np.uint32).copy()
        same = bool((new_own == old_own).all() and (new_own == want(nk)).all() and not any(status))
        ok &= same
        path = "table" if nk >= ctx.get_option("find_table_min_keys") else "ladder"
        out.append("| %d | %d | %s | %s | %s | %.2f | %s |" % (n, nk, ms(t["old"]), ms(t["new"]), path, statistics.median(t["old"]) / statistics.median(t["new"]), same))
    out.append("")

    # ---- 2. both paths forced ----
    out += ["## 2. Both paths forced", "", "| trackers | keys | ladder path ms (`find_table_min_keys` = 2^20 + 1) | table path ms (`find_table_min_keys` = 1) | ladder / table | same owners |",
            "|---|---|---|---|---|---|"]
    crossover = None
    for nk in (16, 32, 64, 128, 256):
        keys = cpx._in(keys_np[:nk].tobytes())
        got = {}

        def forced(value, name, nk=nk, keys=keys, got=got):
            call = new_call(nk, keys)

            def f():
                ctx.set_option("find_table_min_keys", value)
                call()
                got[name] = np.frombuffer(owner, dtype=np.uint32).copy()
            return f
        t = timed([("ladder", forced(NEVER_TABLE, "ladder")), ("table", forced(1, "table"))], a.runs)
        same = bool((got["ladder"] == got["table"]).all() and (got["table"] == want(nk)).all())
        ok &= same
        ml, mt = statistics.median(t["ladder"]), statistics.median(t["table"])
        if crossover is None and mt < ml:
            crossover = nk
        out.append("| %d | %d | %s | %s | %.2f | %s |" % (n, nk, ms(t["ladder"]), ms(t["table"]), ml / mt, same))
    out += ["", "smallest measured power of two at which the table path's median is below the ladder's: %s" % (crossover if crossover else "none up to 256"), ""]

    # ---- 3. kernel times of the table path ----
    nk = KEY_SET
    keys = cpx._in(keys_np[:nk].tobytes())
    ctx.set_option("find_table_min_keys", 1)
    call = new_call(nk, keys)
    call()
    ctx.set_profiling(True)
    ctx.reset_stats()
    call()
    st = {k: ctx.stat(k) for k in ("k_decompress", "k_table_build", "k_fix_build", "k_find_scan")}
    ctx.set_profiling(False)
    pairs = float(n) * nk
    scan_s = st["k_find_scan"]["ms"] / 1e3
    out += ["## 3. Kernel times of the table path, %d trackers x %d keys (profiling on, one call)" % (n, nk), "",
            "| kernel | launches | total ms | ms per chunk |", "|---|---|---|---|"]
    for k, s in st.items():
        out.append("| `%s` | %d | %.2f | %.2f |" % (k, s["launches"], s["ms"], s["ms"] / max(1, s["launches"])))
    fp12 = ctx.bench_fpmul()
    ctx.set_option("bench_field", 28)
    fp28 = ctx.bench_fpmul()
    out += ["", "chunks of %d MiB (option `find_table_mb`); %.3g pairs scanned in %.2f ms = %.3g pairs/s" % (ctx.get_option("find_table_mb"), pairs, 1e3 * scan_s, pairs / scan_s),
            "", "field products of the scan at 32 mixed additions x 10 products per pair (an upper bound: a zero digit is skipped): %.3g products/s;"
            % (pairs * 320 / scan_s),
            "`cpx_bench_fpmul` in the same run: %.3g products/s (32-bit limbs, `bench_field` = 12), %.3g products/s (28-bit-limb table form, `bench_field` = 28)" % (fp12, fp28),
            "", "all routes agree on every owner: %s" % ok]
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
