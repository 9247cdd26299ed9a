"""The host-driven prover (Engine::batch_prove_tables: a lone proof and batches below device_min_batch) of two builds of libcpx.so side by
side in one process, on one GPU.

    python scripts/host_prove_ab.py --base PARENT/libcpx.so [--base-copy COPY/libcpx.so] [--new THIS/libcpx.so] [--rounds 9] [--reps 5] [--out FILE.json]

Two shapes: one proof at ell = 252 and 40 proofs at ell = 28 (the spin-team path).  Per shape and pair of builds: one context of each
library with the same CRS and batch loaded, two warm-up proves each, then `--rounds` rounds that time Context.prove_batch of the two
ALTERNATELY, the order reversed every round (clock drift and neighbours on the machine hit both alike); a round's figure is the mean of
`--reps` consecutive calls, a build's figure the median of its rounds.  With --base-copy (a second copy of the base library under another
path, so that it is loaded as a library of its own) the pair base / copy runs first: the same code against itself; how far its ratio of medians lies
from 1 is the noise band the ratio new / base is read against.  Every proof of every build is compared with the oracle's.  Prints one JSON object; exit
status 1 if any proof differs.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import curdleproofs_amd as cpx   # noqa: E402
from tests.oracle_lib import Oracle   # noqa: E402

SHAPES = [(252, 1), (28, 40)]   # (ell, proofs)


def pair(libs, ell, crs, insts, rounds, reps):
    """libs: two (name, path).  Returns (per-build figures, all proofs equal the oracle's)"""
    cat = lambda key: b"".join(x[key] for x in insts)
    perms = [i for x in insts for i in x["permutation"]]
    perms = (ctypes.c_uint32 * len(perms))(*perms)   # marshalled once, like the byte strings: the timed call is the prove alone
    k, mbl, rand = cat("k"), cat("vec_m_blinders"), cat("prover_rand")
    ctxs = []
    for name, path in libs:
        ctx = cpx.Context(0, lib=path)
        ctx.set_crs(ell, crs)
        ctx.load_batch(*(cat(key) for key in ("vec_R", "vec_S", "vec_T", "vec_U", "M")))
        ctxs.append((name, ctx, []))
    prove = lambda ctx: ctx.prove_batch(perms, k, mbl, rand)
    want = [x["proof"] for x in insts]
    ok = True
    for _, ctx, _ in ctxs:
        for _ in range(2):
            ok &= list(prove(ctx)) == want
    for r in range(rounds):
        for name, ctx, acc in (ctxs if r % 2 == 0 else ctxs[::-1]):
            t0 = time.perf_counter()
            for _ in range(reps):
                proofs = prove(ctx)
            acc.append((time.perf_counter() - t0) / reps * 1e3)
            ok &= list(proofs) == want
    res = {}
    for name, ctx, acc in ctxs:
        q = statistics.quantiles(acc, n=4)
        res[name] = {"median_ms": statistics.median(acc), "q1_ms": q[0], "q3_ms": q[2], "min_ms": min(acc), "max_ms": max(acc), "rounds_ms": [round(t, 4) for t in acc]}
        ctx.close()
    a, b = (res[name]["median_ms"] for name, _ in libs)
    res["second_over_first"] = b / a
    return res, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True)
    ap.add_argument("--base-copy")
    ap.add_argument("--new", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("at least seven rounds")
    new = a.new or cpx._LIB_PATH
    orc = Oracle()
    out = {"rounds": a.rounds, "reps": a.reps, "shapes": []}
    ok = True
    for ell, count in SHAPES:
        crs = orc.generate_crs_points(ell)
        insts = [orc.make_instance(ell, seed, crs) for seed in range(count)]
        shape = {"ell": ell, "proofs": count}
        if a.base_copy:
            shape["base_vs_copy"], good = pair([("base", a.base), ("base_copy", a.base_copy)], ell, crs, insts, a.rounds, a.reps)
            ok &= good
        shape["base_vs_new"], good = pair([("base", a.base), ("new", new)], ell, crs, insts, a.rounds, a.reps)
        ok &= good
        if a.base_copy:   # the band: how far the same code lies from itself, as a ratio of medians (the level drifts from pair to pair, a ratio does not)
            shape["band"] = abs(shape["base_vs_copy"]["second_over_first"] - 1)
            shape["new_inside_band"] = abs(shape["base_vs_new"]["second_over_first"] - 1) <= shape["band"]
        out["shapes"].append(shape)
    out["all_proofs_equal_the_oracles"] = bool(ok)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
