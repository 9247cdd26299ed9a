"""One run of Whisk shuffles through cpx_whisk_verify_shuffle_run against host replay plus cpx_whisk_verify_shuffle_proofs.

    python scripts/shuffle_run_rate.py [--ell 124] [--candidates 16384] [--items 2048] [--runs 7] [--commit ID] [--out profiles/shuffle_run.md]

The run: `--items` blocks over one list of `--candidates` trackers.  The blocks come in waves of candidates // ell: the blocks of a wave touch
pairwise different indices (a random partition), every wave after the first reads what the waves before it wrote.  That keeps the run as
dependent as a chain of blocks is while the library's own batched prover can make the proofs wave by wave (a proof per block from the
oracle would take an hour).  Inputs are seeded (random.Random); every block has its own permutation, k, blinders and draws.

Timed, at the C-ABI with the buffers marshalled beforehand, in ONE process and alternating, --runs times after one warm-up of each:
  run       cpx_whisk_verify_shuffle_run with write-back (the candidate list is loaded again before every call, outside the window)
  replay    the host replay that produces the explicit pre trackers (numpy gathers and scatters over a [candidates][96] byte array)
  explicit  cpx_whisk_verify_shuffle_proofs on those pre trackers
The claim under test: run < replay + explicit by more than the run-to-run spread.  Then one profiled call of each form for the kernel
times (k_decompress, k_run_gather, k_run_commit, k_shuffle_status).  Exit status 1 if a verdict is not CPX_OK, the two forms disagree,
or the list the run call leaves differs from the replay.
"""
import argparse
import ctypes
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import curdleproofs_amd as cpx   # noqa: E402
from curdleproofs_amd import crs as crsmod, params   # noqa: E402

SEED = "shuffle_run_rate"
KERNELS = ("k_decompress", "k_run_gather", "k_run_commit", "k_shuffle_status")


def compress(ctx, aff):
    one = params.fp_to_wire(1)
    return ctx.normalize(b"".join(aff[96 * i:96 * (i + 1)] + one for i in range(len(aff) // 96)), compressed=True)[1]


def make_run(ctx, ell, nc, items, rng):
    """candidates [nc][96], index table [items][ell], post trackers [items][ell][96] and the proofs, made wave by wave"""
    L, h, n = ctx._L, ctx._h, ell + 4
    rec = 48 + ctx.proof_size
    r_g = ctx.scale(params.g1_generator_wire() * nc, params.random_fr_wire(rng, nc))
    k_r_g = ctx.scale(r_g, params.random_fr_wire(rng, nc))
    cr, cs = np.frombuffer(compress(ctx, r_g), np.uint8).reshape(nc, 48), np.frombuffer(compress(ctx, k_r_g), np.uint8).reshape(nc, 48)
    cand = np.concatenate([cr, cs], axis=1)
    lst = cand.copy()
    per_wave = nc // ell
    table = np.zeros((items, ell), np.uint32)
    posts = np.zeros((items, ell, 96), np.uint8)
    proofs = np.zeros((items, rec), np.uint8)
    done = 0
    while done < items:
        c = min(per_wave, items - done)
        order = list(range(nc))
        rng.shuffle(order)
        idx = np.array(order[:c * ell], np.uint32).reshape(c, ell)
        perm = []
        for _ in range(c):
            p = list(range(ell))
            rng.shuffle(p)
            perm += p
        pre = cpx._in(lst[idx.reshape(-1)].tobytes())
        post, pf, st = cpx._out(96 * ell * c), cpx._out(rec * c), (ctypes.c_int * c)()
        ctx._check(L.cpx_whisk_generate_shuffle_proofs(h, c, pre, (ctypes.c_uint32 * (c * ell))(*perm), cpx._in(params.random_fr_wire(rng, c)),
                                                       cpx._in(params.random_fr_wire(rng, 4 * c)), cpx._in(params.random_fr_wire(rng, (3 * n + 9) * c)), post, pf, st))
        assert all(s == cpx.CPX_OK for s in st)
        table[done:done + c] = idx
        posts[done:done + c] = np.frombuffer(bytes(post), np.uint8).reshape(c, ell, 96)
        proofs[done:done + c] = np.frombuffer(bytes(pf), np.uint8).reshape(c, rec)
        lst[idx.reshape(-1)] = posts[done:done + c].reshape(-1, 96)      # (a wave's indices are pairwise different)
        done += c
    return cand, table, posts, proofs


def replay(cand, table, posts):
    """what a caller of the explicit call does: the pre trackers of every block, and the list afterwards"""
    lst = cand.copy()
    pre = np.empty_like(posts)
    for b in range(table.shape[0]):
        pre[b] = lst[table[b]]
        lst[table[b]] = posts[b]
    return pre, lst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ell", type=int, default=124)
    ap.add_argument("--candidates", type=int, default=16384)
    ap.add_argument("--items", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out")
    a = ap.parse_args()
    ell, nc, items = a.ell, a.candidates, a.items
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = cpx.Context(0)
    L, h = ctx._L, ctx._h
    crsmod.crs_from_seed(ctx, ell, SEED)
    rng = random.Random(20261020)
    cand, table, posts, proofs = make_run(ctx, ell, nc, items, rng)
    cand_b = cpx._in(cand.tobytes())
    idx = (ctypes.c_uint32 * (items * ell))(*table.reshape(-1).tolist())
    post_b, proofs_b, rand_b = cpx._in(posts.tobytes()), cpx._in(proofs.tobytes()), cpx._in(params.random_fr_wire(rng, 8 * items))
    v_run, v_exp = (ctypes.c_int * items)(), (ctypes.c_int * items)()
    applied = ctypes.c_size_t(0)
    state = {}

    def load():
        ctx._check(L.cpx_whisk_candidates_load(h, nc, cand_b, None))

    def run_call():
        ctx._check(L.cpx_whisk_verify_shuffle_run(h, items, idx, post_b, proofs_b, rand_b, v_run, ctypes.byref(applied)))

    def replay_call():
        pre, state["list"] = replay(cand, table, posts)
        state["pre"] = cpx._in(pre.tobytes())

    def explicit_call():
        ctx._check(L.cpx_whisk_verify_shuffle_proofs(h, items, state["pre"], post_b, proofs_b, rand_b, v_exp))

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    t = {"load": [], "run": [], "replay": [], "explicit": []}
    for i in range(a.runs + 1):                       # pass 0 warms every shape up and is not counted
        row = dict(load=clock(load), run=clock(run_call), replay=clock(replay_call), explicit=clock(explicit_call))
        if i:
            for k, v in row.items():
                t[k].append(v)
    out = (ctypes.c_uint8 * (96 * nc))()
    ctx._check(L.cpx_whisk_candidates_read(h, 0, nc, out))
    ok = all(v == cpx.CPX_OK for v in v_run) and list(v_run) == list(v_exp) and applied.value == items and bytes(out) == state["list"].tobytes()
    # one profiled call of each form
    ctx.set_profiling(True)
    kern = {}
    for name, fn in (("run", lambda: (load(), ctx.reset_stats(), run_call())), ("explicit", lambda: (ctx.reset_stats(), explicit_call()))):
        fn()
        kern[name] = {k: ctx.stat(k) for k in KERNELS}
    ctx.set_profiling(False)

    med = {k: statistics.median(v) for k, v in t.items()}
    both = [r + e for r, e in zip(t["replay"], t["explicit"])]
    spread = max(max(t["run"]) - min(t["run"]), max(both) - min(both))
    gain = statistics.median(both) - med["run"]
    say("# A run of Whisk shuffles: `cpx_whisk_verify_shuffle_run` against host replay + `cpx_whisk_verify_shuffle_proofs`")
    say()
    say("`scripts/shuffle_run_rate.py`, commit %s, one MI355X, one process, the forms alternating, %d timed passes after one warm-up pass." % (a.commit, a.runs))
    say("ell = %d, %d candidates, %d items (waves of %d blocks on pairwise different indices), proof record %d B, device_min_batch = %d, fix_bits = %d." %
        (ell, nc, items, nc // ell, 48 + ctx.proof_size, ctx.get_option("device_min_batch"), ctx.get_option("fix_bits_effective")))
    say()
    say("| wall time per call, ms | median | min | max |")
    say("|---|---|---|---|")
    for k, label in (("run", "run call (with write-back)"), ("replay", "host replay (numpy)"), ("explicit", "explicit call"), ("load", "candidates_load (outside the run's window)")):
        say("| %s | %.2f | %.2f | %.2f |" % (label, med[k], min(t[k]), max(t[k])))
    say("| host replay + explicit call | %.2f | %.2f | %.2f |" % (statistics.median(both), min(both), max(both)))
    say()
    say("| kernel, ms (units) in one profiled call | run call | explicit call |")
    say("|---|---|---|")
    for k in KERNELS:
        say("| `%s` | %.3f (%d) | %.3f (%d) |" % (k, kern["run"][k]["ms"], kern["run"][k]["units"], kern["explicit"][k]["ms"], kern["explicit"][k]["units"]))
    say()
    say("`k_run_gather` moved %.1f MB, `k_run_commit` %.1f MB (algorithmic bytes)." % (kern["run"]["k_run_gather"]["alg_bytes"] / 1e6, kern["run"]["k_run_commit"]["alg_bytes"] / 1e6))
    say("Run-to-run spread (the larger range of the two sides): %.2f ms.  Median gain of the run call over replay + explicit: %.2f ms (%.1f %%); over the explicit call alone: %.2f ms." %
        (spread, gain, 100 * gain / statistics.median(both), med["explicit"] - med["run"]))
    say("The claim that the run call is faster than replay plus the explicit call by more than the spread is **%s** by this run." % ("confirmed" if gain > spread else "refuted"))
    say("All verdicts CPX_OK, both forms agree, n_applied = items and the resident list equals the replay: %s." % bool(ok))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
