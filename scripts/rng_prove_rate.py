"""What drawing the prover's randomness on the device costs or saves: cpx_batch_prove with page-locked marshalled draws against
cpx_batch_prove_rng (40 bytes of state per proof, the 3n + 9 draws made by k_rng_draw) on the same loaded batch, one context.

    python scripts/rng_prove_rate.py [--ell 252] [--batches 8192,1024] [--runs 9] [--out FILE.md]

For every batch size: one instance (seeded; made with cpx_batch_shuffle) repeated over the batch, one stream per proof split off one parent.
The explicit draws are the ones the streams give (cpx_rng_fr), so both calls must return the same bytes: exit status 1 if they do not or
if a state does not come back where cpx_rng_fr left it.  The two calls alternate; the figures are medians of --runs calls each on the host
clock after one warm-up pair, at the C-ABI with every buffer marshalled beforehand.  Beside them: k_rng_draw's own time from the library's
kernel statistics (a profiled pass of its own), and the time ONE host core takes to draw the same scalars with the same code (rng.hpp
compiled by g++ into a throw-away program; n/a without a compiler).
"""
import argparse
import ctypes
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import curdleproofs_amd as cpx   # noqa: E402
from curdleproofs_amd import crs as crsmod, params   # noqa: E402
from curdleproofs_amd.rng import StdRng   # noqa: E402

SEED = "rng_prove_rate"

HOST_SRC = r"""
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "%s"
using namespace cpx;
int main(int argc, char** argv) {
  const long streams = atol(argv[1]), each = atol(argv[2]);
  RngStream parent(rng_seed_from_u64(1));
  uint32_t acc = 0, fr[8];
  const auto t0 = std::chrono::steady_clock::now();
  for (long s = 0; s < streams; s++) {
    RngStream child(rng_split(parent));
    for (long i = 0; i < each; i++) {
      rng_fr(child, fr);
      acc ^= fr[0];
    }
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("%%.3f %%u\n", ms, acc);
  return 0;
}
"""


def host_draw_ms(streams, each):
    try:
        with tempfile.TemporaryDirectory() as d:
            src, exe = os.path.join(d, "draw.cpp"), os.path.join(d, "draw")
            with open(src, "w") as f:
                f.write(HOST_SRC % os.path.join(ROOT, "curdleproofs_amd", "csrc", "rng.hpp"))
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            return float(subprocess.run([exe, str(streams), str(each)], capture_output=True, text=True, check=True, timeout=600).stdout.split()[0])
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ell", type=int, default=252)
    ap.add_argument("--batches", default="8192,1024")
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = cpx.Context(0)
    L, h = ctx._L, ctx._h
    ell, n = a.ell, a.ell + 4
    nr = 3 * n + 9
    crsmod.crs_from_seed(ctx, ell, SEED)
    psz = ctx.proof_size
    rng = random.Random(20261019)
    vec_r = ctx.scale(params.g1_generator_wire() * ell, params.random_fr_wire(rng, ell))
    vec_s = ctx.scale(vec_r, params.random_fr_wire(rng, ell))
    perm1 = list(range(ell))
    rng.shuffle(perm1)
    k1, mb1 = params.random_fr_wire(rng, 1), params.random_fr_wire(rng, 4)
    vec_t, vec_u, m = ctx.shuffle_batch(vec_r, vec_s, perm1, k1, mb1)
    ok = True
    say("# rng_prove_rate: ell = %d, proof %d B, %d draws (%d B) per proof, runs = %d (median, host clock), device_min_batch = %d, fix_bits = %d" %
        (ell, psz, nr, 32 * nr, a.runs, ctx.get_option("device_min_batch"), ctx.get_option("fix_bits_effective")))
    say("")
    say("| batch | `cpx_batch_prove` ms (uploaded draws) | proofs/s | `cpx_batch_prove_rng` ms | proofs/s | rng / uploaded | `k_rng_draw` ms | one host core, same draws, ms | randomness up, MB: draws / states | min - max ms: uploaded / rng |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    for B in (int(b) for b in a.batches.split(",")):
        ctx.load_batch(vec_r * B, vec_s * B, vec_t * B, vec_u * B, m * B)
        perm, k, mb = ctx.marshal(perm1 * B), ctx.marshal(k1 * B), ctx.marshal(mb1 * B)
        start = b"".join(c.state for c in StdRng.seed_from_u64(1).split(B))
        st = ctx.marshal(start)
        draws = ctx.marshal(bytes(32 * nr * B))
        ctx._check(L.cpx_rng_fr(h, B, st, nr, draws))
        after = bytes(st)
        out_a, out_b = ctx.marshal(bytes(B * psz)), ctx.marshal(bytes(B * psz))

        def explicit():
            ctx._check(L.cpx_batch_prove(h, perm, k, mb, draws, out_a))

        def on_device():
            ctypes.memmove(st, start, len(start))
            ctx._check(L.cpx_batch_prove_rng(h, perm, k, mb, st, out_b))

        explicit(), on_device()
        ok &= bytes(out_a) == bytes(out_b) and bytes(st) == after
        ta, tb = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            explicit()
            t1 = time.perf_counter()
            on_device()
            t2 = time.perf_counter()
            ta.append(t1 - t0)
            tb.append(t2 - t1)
        spread = "%.1f - %.1f / %.1f - %.1f" % (1e3 * min(ta), 1e3 * max(ta), 1e3 * min(tb), 1e3 * max(tb))
        ta, tb = statistics.median(ta), statistics.median(tb)
        ctx.set_profiling(True)
        ctx.reset_stats()
        on_device()
        kst = ctx.stat("k_rng_draw")
        ctx.set_profiling(False)
        hm = host_draw_ms(B, nr)
        say("| %d | %.2f | %.0f | %.2f | %.0f | %.4f | %.3f | %s | %.1f / %.2f | %s |" %
            (B, 1e3 * ta, B / ta, 1e3 * tb, B / tb, tb / ta, kst["ms"] / max(kst["launches"], 1), "n/a" if hm is None else "%.0f" % hm, 32e-6 * nr * B, 40e-6 * B, spread))
    say("")
    say("same proof bytes and states from both calls: %s" % bool(ok))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
