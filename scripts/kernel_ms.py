"""Per-kernel milliseconds of one prove and one verify of `--proofs` copies of one oracle instance on ONE context with serial_streams = 1
(every stream's work in line on the main stream: each kernel's event-timed duration is its own and a pass is the plain sum of its
kernels), from the engine's statistics.  Two passes (the process's first, "warm", then "timed"); every proof is compared with the
oracle's bytes and verified.  Prints one JSON object; with --out also writes it.
  python scripts/kernel_ms.py --opt rs_from_tables=0 --out kernel_ms_rs0.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=8192)
    ap.add_argument("--ell", type=int, default=252)
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import curdleproofs_amd as cpx
    from tests.oracle_lib import Oracle
    orc = Oracle()
    crs = orc.generate_crs_points(args.ell)
    inst = orc.make_instance(args.ell, 0, crs)
    opts = {"serial_streams": 1}
    opts.update((k, int(v)) for k, v in (o.split("=") for o in args.opt))
    c = cpx.Context(0, options=opts)
    c.set_crs(args.ell, crs)
    nb = args.proofs
    c.load_batch(*(inst[k] * nb for k in ("vec_R", "vec_S", "vec_T", "vec_U", "M")))
    perm = c.marshal(list(inst["permutation"]) * nb)
    k, mbl, prand, vrand = (inst[x] * nb for x in ("k", "vec_m_blinders", "prover_rand", "verifier_rand"))
    c.set_profiling(True)
    names = set(c.KERNELS) | {"k_smul_quad"}
    res = {"options": opts, "proofs": nb, "ell": args.ell, "tbl_segments_effective": None}

    def taken():
        out = {}
        for name in sorted(names):
            s = c.stat(name)
            if s["launches"]:
                out[name] = {"launches": s["launches"], "ms": round(s["ms"], 3), "units": s["units"]}
        out["all_kernels_ms"] = round(sum(v["ms"] for n, v in out.items() if n.startswith("k_")), 3)
        return out

    for tag in ("warm", "timed"):
        c.reset_stats()
        proofs = c.prove_batch(perm, k, mbl, prand)
        prove = taken()
        c.reset_stats()
        verdicts = c.verify_batch(proofs, vrand)
        res[tag] = {"all_equal_oracle": all(p == inst["proof"] for p in proofs), "all_verified": verdicts == [cpx.CPX_OK] * nb, "prove": prove, "verify": taken()}
    res["tbl_segments_effective"] = c.get_option("tbl_segments_effective")
    import ctypes
    free_b, total_b = ctypes.c_size_t(0), ctypes.c_size_t(0)   # (the HIP runtime the library has loaded: with the batch and all scratch resident)
    try:
        if ctypes.CDLL("libamdhip64.so").hipMemGetInfo(ctypes.byref(free_b), ctypes.byref(total_b)) == 0:
            res["hbm_used_gb"] = round((total_b.value - free_b.value) / 1e9, 2)
    except OSError:
        res["hbm_used_gb"] = None
    c.close()
    line = json.dumps(res, indent=1, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
