"""The grouped check of tracker proofs (cpx_whisk_verify_tracker_proofs_grouped) against the per-item call (cpx_whisk_verify_tracker_proofs)
on one context, in one process.

    python scripts/tracker_grouped_rate.py [--counts 64,1024,16384] [--runs 5] [--wrong 16384] [--out FILE.json]

Inputs are seeded (params.random_fr_wire with random.Random: reproducible, CSPRNG-free), the weights included.  Per shape: one warm-up of
each call, then `--runs` rounds that time the two calls ALTERNATELY at the C-ABI with the buffers marshalled beforehand (clock drift and
neighbours on the machine hit both alike); the medians are reported and the verdicts compared.  Two more shapes at `--wrong` items: one
wrong item, and one wrong item in every hundred (s + 1: decodable, fails both relations' sum).  With profiling on, one more call per shape
gives the per-kernel times (Context.stat).  Prints one JSON object; exit status 1 if the two calls disagree anywhere or a valid item is not
CPX_OK.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import curdleproofs_amd as cpx   # noqa: E402
from curdleproofs_amd import params   # noqa: E402
from tracker_proof_rate import make_inputs   # noqa: E402

R_ = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
KERNELS = ("k_decompress", "k_tracker_challenge", "k_tracker_relations", "k_tracker_check_scalars", "k_msm_tblw<2, true>", "k_reduce_sets", "k_msm_tail",
           "k_tracker_gather")


def spoil(proofs, items):
    """s + 1 in the listed proofs"""
    b = bytearray(proofs)
    for i in items:
        s = (int.from_bytes(b[128 * i + 96:128 * (i + 1)], "little") + 1) % R_
        b[128 * i + 96:128 * (i + 1)] = s.to_bytes(32, "little")
    return bytes(b)


def measure(ctx, n, trackers, kcs, proofs, weights, wrong, runs):
    L, h = ctx._L, ctx._h
    tr, kc, pf, w = (cpx._in(x) for x in (trackers[:96 * n], kcs[:48 * n], spoil(proofs[:128 * n], wrong), weights[:64 * n]))
    v_item, v_grp = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    rechecked = ctypes.c_size_t(0)
    item = lambda: ctx._check(L.cpx_whisk_verify_tracker_proofs(h, n, tr, kc, pf, v_item))
    grp = lambda: ctx._check(L.cpx_whisk_verify_tracker_proofs_grouped(h, n, tr, kc, pf, w, v_grp, ctypes.byref(rechecked)))
    item()   # warm-up
    grp()
    t_item, t_grp = [], []
    for _ in range(runs):
        for fn, acc in ((item, t_item), (grp, t_grp)):
            t0 = time.perf_counter()
            fn()
            acc.append(time.perf_counter() - t0)
    wrong = set(wrong)
    want = [cpx.CPX_ERR_VERIFY if i in wrong else cpx.CPX_OK for i in range(n)]
    ok = list(v_item) == want and list(v_grp) == want
    ti, tg = statistics.median(t_item), statistics.median(t_grp)
    kernel_ms = {}
    ctx.set_profiling(True)
    for name, fn in (("per_item", item), ("grouped", grp)):
        ctx.reset_stats()
        fn()
        kernel_ms[name] = {k: round(ctx.stat(k)["ms"], 4) for k in KERNELS if ctx.stat(k)["launches"]}
    ctx.set_profiling(False)
    return {"items": n, "wrong_items": len(wrong), "per_item_ms": ti * 1e3, "grouped_ms": tg * 1e3, "per_item_proofs_per_s": n / ti, "grouped_proofs_per_s": n / tg,
            "grouped_speedup": ti / tg, "n_rechecked": rechecked.value, "verdicts_agree_and_as_expected": ok, "kernel_ms": kernel_ms}, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="64,1024,16384")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--wrong", type=int, default=16384)
    ap.add_argument("--out")
    a = ap.parse_args()
    counts = [int(c) for c in a.counts.split(",")]
    nmax = max(counts + [a.wrong])
    ctx = cpx.Context(0)
    trackers, kcs, ks, bs = make_inputs(ctx, nmax)
    proofs, st = cpx._out(128 * nmax), (ctypes.c_int * nmax)()
    ctx._check(ctx._L.cpx_whisk_generate_tracker_proofs(ctx._h, nmax, cpx._in(trackers), cpx._in(ks), cpx._in(bs), proofs, st))
    proofs = bytes(proofs)
    weights = params.random_fr_wire(random.Random(20261020), 2 * nmax)
    res = {"runs": a.runs, "locate_groups_max": ctx.get_option("locate_groups_max"), "valid": [], "with_wrong_items": []}
    ok = all(s == cpx.CPX_OK for s in st)
    for n in counts:
        r, good = measure(ctx, n, trackers, kcs, proofs, weights, [], a.runs)
        res["valid"].append(r)
        ok &= good
    for wrong in ([a.wrong // 2], list(range(50, a.wrong, 100))):
        r, good = measure(ctx, a.wrong, trackers, kcs, proofs, weights, wrong, a.runs)
        res["with_wrong_items"].append(r)
        ok &= good
    res["all_results_as_expected"] = bool(ok)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
