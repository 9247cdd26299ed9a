"""curdleproofs_amd — MI355X (gfx950) core for the Curdleproofs shuffle argument's G1 hot path.

Python mirror of the reference's interface for this path (asn-d6/curdleproofs):

    util::msm / msm_from_projective           -> Context.msm / Context.msm_from_projective
    the fold / rescale loops                  -> Context.fold / Context.scale
    msm_accumulator::MsmAccumulator           -> MsmAccumulator
    CurdleproofsCrs::from_points              -> Context.set_crs
    CurdleproofsProof::{new, verify}          -> Context.prove_batch / Context.verify_batch
                                                 (CurdleproofsProof.new / .verify for one instance)

All of it is a thin ctypes layer over the C-ABI in include/cpx.h (curdleproofs_amd/_lib/libcpx.so).
There is no CPU implementation behind these calls: if the HIP library or a GPU is missing they raise.
Byte layouts are arkworks' in-memory limbs (Fr 32 B, affine 96 B, Jacobian 144 B); see include/cpx.h.
"""
import ctypes
import os

# eight hardware queues for the HIP streams of this process (the runtime's default of four lets two streams of one engine context share a
# queue in about half of the runs of a two-context process: capi.cpp); read by the runtime at its first call, so it is set
# as early as this package is imported — libcpx.so sets it again when it is loaded — and a value the caller exported wins
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

from .build import LIB as _LIB_PATH

FR = 32
AFF = 96
JAC = 144
N_BLINDERS = 4   # reference src/lib.rs:35
TRANSCRIPT_BYTES = 216   # a transcript state: 25 Keccak lanes, pos, pos_begin as 27 u64 LE (include/cpx.h)

CPX_OK = 0
CPX_ERR_ARG = -1
CPX_ERR_NOT_POW2 = -2
CPX_ERR_HIP = -3
CPX_ERR_VERIFY = -4
CPX_ERR_DESERIALIZE = -5
CPX_ERR_STATE = -6
CPX_ERR_INTERNAL = -7
CPX_NO_OWNER = 0xffffffff   # cpx_whisk_find_trackers: no key opens the tracker

_ERRNAMES = {CPX_ERR_ARG: "bad argument", CPX_ERR_NOT_POW2: "ell + 4 is not a power of two", CPX_ERR_HIP: "HIP failure",
             CPX_ERR_VERIFY: "verification failed", CPX_ERR_DESERIALIZE: "deserialization failed",
             CPX_ERR_STATE: "call order (CRS / batch not set)", CPX_ERR_INTERNAL: "internal error"}


class CpxError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        super().__init__("cpx error %d (%s) %s" % (code, _ERRNAMES.get(code, "?"), detail))


class ProofError(CpxError):
    """Mirror of the reference's ProofError::VerificationError (src/errors.rs:9)."""


_lib = None
_libs = {}   # realpath -> loaded library (the default one and build variants for A/B runs)

EXPORTS = [
    "cpx_host_alloc", "cpx_host_free", "cpx_ctx_create", "cpx_ctx_destroy", "cpx_last_error", "cpx_device_count", "cpx_ctx_set_option", "cpx_ctx_get_option", "cpx_ctx_set_crs", "cpx_crs_sums", "cpx_proof_size", "cpx_batch_size",
    "cpx_g1_msm", "cpx_g1_msm_jac", "cpx_g1_fold", "cpx_g1_scale", "cpx_g1_msm_many", "cpx_g1_fold_many", "cpx_ipa_rounds", "cpx_same_msm_rounds", "cpx_ipa_verify", "cpx_same_msm_verify", "cpx_ipa_prove", "cpx_same_msm_prove", "cpx_ipa_prove_rng", "cpx_same_msm_prove_rng", "cpx_gprod_prove", "cpx_gprod_prove_rng", "cpx_gprod_verify", "cpx_same_perm_prove", "cpx_same_perm_prove_rng", "cpx_same_perm_verify",
    "cpx_transcript_new", "cpx_transcript_append_message", "cpx_transcript_append_scalar", "cpx_transcript_challenge_bytes", "cpx_transcript_challenge_scalar",
    "cpx_g1_normalize", "cpx_g1_decompress", "cpx_g1_decompress_status",
    "cpx_accum_new", "cpx_accum_free", "cpx_accum_check", "cpx_accum_verify",
    "cpx_batch_load", "cpx_batch_load_begin", "cpx_batch_load_end", "cpx_batch_prove", "cpx_batch_verify", "cpx_batch_verify_fused", "cpx_batch_verify_grouped", "cpx_g1_sum_jac",
    "cpx_whisk_generate_shuffle_proof", "cpx_whisk_is_valid_shuffle_proof", "cpx_whisk_generate_tracker_proof", "cpx_whisk_is_valid_tracker_proof",
    "cpx_whisk_generate_tracker_proofs", "cpx_whisk_verify_tracker_proofs", "cpx_whisk_verify_tracker_proofs_fused", "cpx_whisk_verify_tracker_proofs_grouped", "cpx_g1_generator_mul", "cpx_whisk_trackers_from_k_r", "cpx_whisk_find_trackers",
    "cpx_batch_shuffle", "cpx_whisk_generate_shuffle_proofs", "cpx_whisk_verify_shuffle_proofs", "cpx_whisk_verify_shuffle_proofs_grouped",
    "cpx_whisk_candidates_load", "cpx_whisk_candidates_size", "cpx_whisk_candidates_read", "cpx_whisk_verify_shuffle_run", "cpx_whisk_verify_shuffle_run_grouped",
    "cpx_rng_from_u64", "cpx_rng_split", "cpx_rng_fr", "cpx_rng_shuffle_draws", "cpx_whisk_generate_shuffle_proofs_rng", "cpx_batch_prove_rng",
    "cpx_rng_g1", "cpx_rng_instance_draws", "cpx_crs_generate", "cpx_g1_clear_cofactor",
    "cpx_set_profiling", "cpx_reset_stats", "cpx_get_stat", "cpx_set_host_threads", "cpx_bench_fpmul",
]


def load_library(path=None):
    """Loads libcpx.so; raises if it has not been built (python -m curdleproofs_amd.build).  `path`: another build of the
    library (curdleproofs_amd.build.build_variant) beside the default one in the same process — bench.py --ab-lib runs contexts of
    both on the same GPU, pass by pass; every library is loaded once and keeps its own CRS tables."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    if path is not None and os.path.realpath(path) in _libs:
        return _libs[os.path.realpath(path)]
    default = path is None
    path = path or os.environ.get("CPX_LIB", _LIB_PATH)   # CPX_LIB: experimental build variant as THE library of the process
    if not os.path.exists(path):
        raise ImportError("curdleproofs_amd: %s is missing — build it with `python -m curdleproofs_amd.build` "
                          "(hipcc, gfx950). There is no CPU fallback." % _LIB_PATH)
    L = ctypes.CDLL(path)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.cpx_host_alloc.argtypes = [sz]
    L.cpx_host_alloc.restype = vp
    L.cpx_host_free.argtypes = [vp]
    L.cpx_host_free.restype = None
    L.cpx_ctx_create.argtypes = [ci, ctypes.POINTER(vp)]
    L.cpx_ctx_destroy.argtypes = [vp]
    L.cpx_ctx_destroy.restype = None
    L.cpx_last_error.argtypes = [vp]
    L.cpx_last_error.restype = ctypes.c_char_p
    L.cpx_device_count.argtypes = []
    L.cpx_ctx_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_longlong]
    L.cpx_ctx_get_option.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong)]
    L.cpx_ctx_set_crs.argtypes = [vp, sz, vp, sz]
    L.cpx_crs_sums.argtypes = [vp, vp, vp]
    L.cpx_proof_size.argtypes = [vp]
    L.cpx_proof_size.restype = sz
    L.cpx_batch_size.argtypes = [vp]
    L.cpx_batch_size.restype = sz
    L.cpx_g1_msm.argtypes = [vp, vp, vp, sz, vp]
    L.cpx_g1_msm_jac.argtypes = [vp, vp, vp, sz, vp]
    L.cpx_g1_fold.argtypes = [vp, vp, vp, vp, sz]
    L.cpx_g1_scale.argtypes = [vp, vp, vp, sz, sz, vp]
    L.cpx_g1_msm_many.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.cpx_g1_fold_many.argtypes = [vp, sz, sz, vp, vp, vp]
    L.cpx_g1_normalize.argtypes = [vp, vp, sz, vp, vp]
    L.cpx_ipa_rounds.argtypes = [vp, sz, sz] + [vp] * 10
    L.cpx_same_msm_rounds.argtypes = [vp, sz, sz] + [vp] * 9
    L.cpx_ipa_verify.argtypes = [vp, sz, sz] + [vp] * 11
    L.cpx_same_msm_verify.argtypes = [vp, sz, sz] + [vp] * 11
    if hasattr(L, "cpx_ipa_prove"):   # (an older build loaded beside this one for an A/B run, scripts/subarg_prove_timing.py, lacks the four)
        L.cpx_ipa_prove.argtypes = [vp, sz, sz] + [vp] * 13
        L.cpx_ipa_prove_rng.argtypes = [vp, sz, sz] + [vp] * 13
        L.cpx_same_msm_prove.argtypes = [vp, sz, sz] + [vp] * 12
        L.cpx_same_msm_prove_rng.argtypes = [vp, sz, sz] + [vp] * 12
    if hasattr(L, "cpx_gprod_prove"):   # (likewise: scripts/gprod_timing.py)
        L.cpx_gprod_prove.argtypes = [vp, sz, sz, sz] + [vp] * 12
        L.cpx_gprod_prove_rng.argtypes = [vp, sz, sz, sz] + [vp] * 12
        L.cpx_gprod_verify.argtypes = [vp, sz, sz, sz] + [vp] * 12
    if hasattr(L, "cpx_same_perm_prove"):   # (likewise: scripts/same_perm_timing.py)
        L.cpx_same_perm_prove.argtypes = [vp, sz, sz, sz] + [vp] * 14
        L.cpx_same_perm_prove_rng.argtypes = [vp, sz, sz, sz] + [vp] * 14
        L.cpx_same_perm_verify.argtypes = [vp, sz, sz, sz] + [vp] * 13
    L.cpx_transcript_new.argtypes = [vp, sz, vp]
    L.cpx_transcript_append_message.argtypes = [vp, vp, sz, vp, sz]
    L.cpx_transcript_append_scalar.argtypes = [vp, vp, sz, vp]
    L.cpx_transcript_challenge_bytes.argtypes = [vp, vp, sz, vp, sz]
    L.cpx_transcript_challenge_scalar.argtypes = [vp, vp, sz, vp]
    L.cpx_g1_decompress.argtypes = [vp, vp, sz, vp, ci]
    L.cpx_g1_decompress_status.argtypes = [vp, vp, sz, vp, ci, vp]
    L.cpx_accum_new.argtypes = [vp, ctypes.POINTER(vp)]
    L.cpx_accum_free.argtypes = [vp]
    L.cpx_accum_free.restype = None
    L.cpx_accum_check.argtypes = [vp, vp, vp, vp, sz, vp]
    L.cpx_accum_verify.argtypes = [vp]
    L.cpx_batch_load.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.cpx_batch_load_begin.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.cpx_batch_load_end.argtypes = [vp]
    L.cpx_batch_prove.argtypes = [vp, vp, vp, vp, vp, vp]
    L.cpx_batch_verify.argtypes = [vp, vp, vp, vp]
    L.cpx_set_profiling.argtypes = [vp, ci]
    L.cpx_reset_stats.argtypes = [vp]
    L.cpx_get_stat.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double),
                               ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.cpx_batch_verify_fused.argtypes = [vp, vp, vp, vp, ctypes.POINTER(ci)]
    L.cpx_batch_verify_grouped.argtypes = [vp, vp, vp, vp, ctypes.POINTER(sz)]
    L.cpx_g1_sum_jac.argtypes = [vp, vp, sz, vp, ctypes.POINTER(ci)]
    L.cpx_set_host_threads.argtypes = [vp, ci]
    L.cpx_whisk_generate_shuffle_proof.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.cpx_whisk_is_valid_shuffle_proof.argtypes = [vp, vp, vp, vp, vp, ctypes.POINTER(ci)]
    L.cpx_whisk_generate_tracker_proof.argtypes = [vp, vp, vp, vp, vp]
    L.cpx_whisk_is_valid_tracker_proof.argtypes = [vp, vp, vp, vp, ctypes.POINTER(ci)]
    L.cpx_whisk_generate_tracker_proofs.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.cpx_whisk_verify_tracker_proofs.argtypes = [vp, sz, vp, vp, vp, vp]
    L.cpx_whisk_verify_tracker_proofs_fused.argtypes = [vp, sz, vp, vp, vp, vp, vp, ctypes.POINTER(ci)]
    L.cpx_whisk_verify_tracker_proofs_grouped.argtypes = [vp, sz, vp, vp, vp, vp, vp, ctypes.POINTER(sz)]
    L.cpx_g1_generator_mul.argtypes = [vp, sz, vp, vp, vp]
    L.cpx_whisk_trackers_from_k_r.argtypes = [vp, sz, vp, vp, vp, vp]
    L.cpx_whisk_find_trackers.argtypes = [vp, sz, vp, sz, vp, vp, vp]
    L.cpx_batch_shuffle.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    L.cpx_whisk_generate_shuffle_proofs.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    L.cpx_whisk_verify_shuffle_proofs.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.cpx_whisk_verify_shuffle_proofs_grouped.argtypes = [vp, sz, vp, vp, vp, vp, vp, ctypes.POINTER(sz)]
    L.cpx_whisk_candidates_load.argtypes = [vp, sz, vp, vp]
    L.cpx_whisk_candidates_size.argtypes = [vp]
    L.cpx_whisk_candidates_size.restype = sz
    L.cpx_whisk_candidates_read.argtypes = [vp, sz, sz, vp]
    L.cpx_whisk_verify_shuffle_run.argtypes = [vp, sz, vp, vp, vp, vp, vp, ctypes.POINTER(sz)]
    L.cpx_whisk_verify_shuffle_run_grouped.argtypes = [vp, sz, vp, vp, vp, vp, vp, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    L.cpx_bench_fpmul.argtypes = [vp, ci, ci, ci, ctypes.POINTER(ctypes.c_double)]
    L.cpx_rng_from_u64.argtypes = [ctypes.c_uint64, vp]
    L.cpx_rng_split.argtypes = [vp, sz, vp]
    L.cpx_rng_fr.argtypes = [vp, sz, vp, sz, vp]
    L.cpx_rng_shuffle_draws.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.cpx_whisk_generate_shuffle_proofs_rng.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.cpx_batch_prove_rng.argtypes = [vp, vp, vp, vp, vp, vp]
    L.cpx_rng_g1.argtypes = [vp, sz, vp, sz, vp, vp]
    L.cpx_rng_instance_draws.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.cpx_crs_generate.argtypes = [vp, sz, vp, vp]
    L.cpx_g1_clear_cofactor.argtypes = [vp, vp, sz, vp]
    _libs[os.path.realpath(path)] = L
    if default:
        _lib = L
    return L


def device_count():
    return load_library().cpx_device_count()


def _in(b):
    if isinstance(b, ctypes.Array):   # already marshalled (see Context.marshal): no copy
        return b
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) if len(b) else b"\0")


def _len(b):
    return ctypes.sizeof(b) if isinstance(b, ctypes.Array) else len(b)


def _out(n):
    return (ctypes.c_uint8 * max(n, 1))()


class _PinnedOwner:
    def __init__(self, L, addr):
        self.L, self.addr = L, addr

    def __del__(self):
        try:
            self.L.cpx_host_free(self.addr)
        except Exception:
            pass


def _pinned_array(ctype, n):
    """ctypes array of n elements in page-locked host memory (falls back to ordinary memory if the allocation fails)."""
    L = load_library()
    nbytes = ctypes.sizeof(ctype) * n
    addr = None if os.environ.get("CPX_PINNED") == "0" else L.cpx_host_alloc(nbytes)   # CPX_PINNED=0: ordinary memory (A/B runs)
    if not addr:
        return (ctype * n)()
    arr = (ctype * n).from_address(addr)
    arr._cpx_owner = _PinnedOwner(L, addr)   # freed when the array object goes away
    return arr


class Context:
    """One HIP device + stream + device-resident CRS (cpx_ctx)."""

    def __init__(self, device=0, options=None, lib=None):
        self._L = load_library(lib)
        h = ctypes.c_void_p()
        rc = self._L.cpx_ctx_create(device, ctypes.byref(h))
        if rc != CPX_OK:
            raise CpxError(rc, "cpx_ctx_create(device=%d): no usable MI355X/HIP device" % device)
        self._h = h
        self.ell = None
        try:
            for key, value in (options or {}).items():
                self.set_option(key, value)
        except Exception:   # an unknown key / a value out of range: do not leak the native context (streams, engine) of the half-built object
            self.close()
            raise

    @property
    def batch(self):
        """instances currently loaded into the engine (cpx_batch_size): the library is the one source of truth — a Whisk shuffle call
        replaces the loaded batch by its single instance, also when it fails half-way"""
        return self._L.cpx_batch_size(self._h) if getattr(self, "_h", None) else 0

    def set_option(self, key, value):
        """Per-context tunable (include/cpx.h cpx_ctx_set_option; keys: curdleproofs_amd/csrc/kernels.h `Options`)."""
        self._check(self._L.cpx_ctx_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = ctypes.c_longlong(0)
        self._check(self._L.cpx_ctx_get_option(self._h, key.encode(), ctypes.byref(v)))
        return v.value

    def close(self):
        if getattr(self, "_h", None):
            self._L.cpx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != CPX_OK:
            detail = self._L.cpx_last_error(self._h).decode(errors="replace")
            raise (ProofError if rc == CPX_ERR_VERIFY else CpxError)(rc, detail)

    # ---- CRS (crs.rs:37-58) ----
    def set_crs(self, ell, points):
        if len(points) % AFF:
            raise ValueError("CRS points: 96 bytes per affine point")
        # crs.rs:40-42 "not enough points" is reported by the library (CPX_ERR_ARG); surplus points are ignored like the reference's slicing
        self._check(self._L.cpx_ctx_set_crs(self._h, ell, _in(points), len(points) // AFF))
        points = points[:AFF * (ell + 7)]
        self.ell = ell
        self.n = ell + N_BLINDERS
        self.crs_points = bytes(points)

    def crs_sums(self):
        g, h = _out(AFF), _out(AFF)
        self._check(self._L.cpx_crs_sums(self._h, g, h))
        return bytes(g), bytes(h)

    @property
    def proof_size(self):
        return self._L.cpx_proof_size(self._h)

    # ---- tier 0 ----
    def msm(self, bases, scalars):
        """util.rs:19-22; panics in the reference on a length mismatch -> ValueError here."""
        n = len(scalars) // FR
        if len(bases) != AFF * n or len(scalars) != FR * n:
            raise ValueError("number of points != number of scalars")
        o = _out(JAC)
        self._check(self._L.cpx_g1_msm(self._h, _in(bases), _in(scalars), n, o))
        return bytes(o)

    def msm_from_projective(self, bases_jac, scalars):
        n = len(scalars) // FR
        if len(bases_jac) != JAC * n:
            raise ValueError("number of points != number of scalars")
        o = _out(JAC)
        self._check(self._L.cpx_g1_msm_jac(self._h, _in(bases_jac), _in(scalars), n, o))
        return bytes(o)

    def fold(self, PL, PR, gamma):
        half = len(PL) // AFF
        if len(PR) != len(PL) or len(PL) % AFF or len(gamma) != FR:
            raise ValueError("fold: PL / PR must hold the same number of affine points, gamma one scalar")
        b = _in(PL)
        self._check(self._L.cpx_g1_fold(self._h, b, _in(PR), _in(gamma), half))
        return bytes(b)[: AFF * half]

    def scale(self, P, scalars):
        n = len(P) // AFF
        if len(P) % AFF or len(scalars) not in (FR, FR * n):
            raise ValueError("scale: one shared scalar or one scalar per point")
        stride = 0 if len(scalars) == FR else FR
        o = _out(AFF * n)
        self._check(self._L.cpx_g1_scale(self._h, _in(P), _in(scalars), stride, n, o))
        return bytes(o)[: AFF * n]

    def msm_many(self, bases_list, scalars_list, compressed=False):
        """util.rs:19-22 for every (bases, scalars) pair of the lists in ONE call (cpx_g1_msm_many: the cross terms of a log round,
        inner_product_argument.rs:158-161, same_multiscalar_argument.rs:107-112); the lengths may differ, an empty pair gives the identity.
        Returns the list of 144-byte Jacobian results, or (that list, the list of 48-byte encodings)."""
        if len(bases_list) != len(scalars_list):
            raise ValueError("msm_many: one scalar vector per base vector")
        lens = []
        for b, s in zip(bases_list, scalars_list):
            n = len(s) // FR
            if len(b) != AFF * n or len(s) != FR * n:
                raise ValueError("number of points != number of scalars")
            lens.append(n)
        count = len(lens)
        if not count:
            return ([], []) if compressed else []
        la = (ctypes.c_uint32 * count)(*lens)
        o, c = _out(JAC * count), _out(48 * count)
        self._check(self._L.cpx_g1_msm_many(self._h, count, la, _in(b"".join(bytes(b) for b in bases_list)), _in(b"".join(bytes(s) for s in scalars_list)),
                                            o, c if compressed else None))
        jac = [bytes(o)[JAC * i: JAC * (i + 1)] for i in range(count)]
        return (jac, [bytes(c)[48 * i: 48 * (i + 1)] for i in range(count)]) if compressed else jac

    def fold_many(self, PL_list, PR_list, gammas):
        """PL[f][i] + gammas[f] * PR[f][i], affine, for every family f in ONE call (cpx_g1_fold_many: the basis folds of a log round,
        inner_product_argument.rs:177-178, same_multiscalar_argument.rs:128-130).  Every vector holds the same number of points;
        gammas: one 32-byte scalar per family (a list, or the scalars back to back).  Returns the list of folded vectors."""
        if not isinstance(gammas, (bytes, bytearray)):
            if any(len(g) != FR for g in gammas):
                raise ValueError("fold_many: 32 bytes per gamma")
            gammas = b"".join(bytes(g) for g in gammas)
        families = len(PL_list)
        if len(PR_list) != families or len(gammas) != FR * families:
            raise ValueError("fold_many: one PR vector and one gamma per PL vector")
        if not families:
            return []
        size = len(PL_list[0])
        if size % AFF or any(len(v) != size for v in PL_list) or any(len(v) != size for v in PR_list):
            raise ValueError("fold_many: every vector must hold the same number of affine points")
        half = size // AFF
        b = _in(b"".join(bytes(v) for v in PL_list))
        self._check(self._L.cpx_g1_fold_many(self._h, families, half, b, _in(b"".join(bytes(v) for v in PR_list)), _in(gammas)))
        return [bytes(b)[size * f: size * (f + 1)] for f in range(families)]

    def _loop_rounds(self, fn, terms, count, n, inputs, nvec, states, affine):
        if count < 0 or n < 0:
            raise ValueError("count and n are not negative")
        L = max(n.bit_length() - 1, 0)
        if len(states) != count * TRANSCRIPT_BYTES:
            raise ValueError("one 216-byte transcript state per item")
        st = (ctypes.c_uint8 * max(len(states), 1)).from_buffer_copy(bytes(states) if count else b"\0")   # in/out: a copy, the caller's stay
        comp, aff = _out(count * L * terms * 48), _out(count * L * terms * AFF)
        fin, gam = _out(count * nvec * FR), _out(count * L * FR)
        self._check(fn(self._h, count, n, *[_in(b) for b in inputs], st, comp, aff if affine else None, fin, gam))
        out = dict(states=bytes(st)[:count * TRANSCRIPT_BYTES], compressed=bytes(comp)[:count * L * terms * 48], finals=bytes(fin)[:count * nvec * FR],
                   gammas=bytes(gam)[:count * L * FR])
        if affine:
            out["affine"] = bytes(aff)[:count * L * terms * AFF]
        return out

    def ipa_rounds(self, n, G, G_prime, H, vec_c, vec_d, states, affine=False):
        """inner_product_argument.rs:150-186 for len(H) // 96 independent items of n elements in ONE call (cpx_ipa_rounds): all log2 n
        rounds on the device, transcript included.  G, G_prime: the bases as they enter the loop, item after item; H: the loop's point
        (crs_H * beta) per item; vec_c, vec_d: the vectors as they enter the loop; states: the 216-byte transcript states at loop entry
        (curdleproofs_amd.transcript.Transcript.state).  Returns a dict: "states" (advanced by every round), "compressed" (per item and
        round L_C, L_D, R_C, R_D, 48 bytes each), "finals" (per item c_final, d_final), "gammas", and with affine=True "affine"."""
        count = len(H) // AFF
        if len(H) != count * AFF or len(G) != count * n * AFF or len(G_prime) != count * n * AFF or len(vec_c) != count * n * FR or len(vec_d) != count * n * FR:
            raise ValueError("ipa_rounds: per item n points in G and G_prime, one point H, n scalars in vec_c and vec_d")
        return self._loop_rounds(self._L.cpx_ipa_rounds, 4, count, n, (G, G_prime, H, vec_c, vec_d), 2, states, affine)

    def same_msm_rounds(self, n, G, T, U, vec_x, states, affine=False):
        """same_multiscalar_argument.rs:99-136 likewise (cpx_same_msm_rounds), len(states) // 216 items: per round L_A, L_T, L_U, R_A,
        R_T, R_U; "finals" holds x_final per item."""
        count = len(states) // TRANSCRIPT_BYTES
        if any(len(v) != count * n * AFF for v in (G, T, U)) or len(vec_x) != count * n * FR:
            raise ValueError("same_msm_rounds: per item n points in G, T and U and n scalars in vec_x")
        return self._loop_rounds(self._L.cpx_same_msm_rounds, 6, count, n, (G, T, U, vec_x), 1, states, affine)

    def _subarg_verify(self, fn, name, count, n, points, scalars, proofs, rand, states, checks, nchal, proof_bytes, challenges):
        if n < 0:
            raise ValueError("n is not negative")
        if len(states) != count * TRANSCRIPT_BYTES or len(proofs) != count * proof_bytes or len(rand) != count * checks * FR:
            raise ValueError("%s: per item one 216-byte transcript state, %d proof bytes and %d random factors" % (name, proof_bytes, checks))
        st = (ctypes.c_uint8 * max(len(states), 1)).from_buffer_copy(bytes(states) if count else b"\0")   # in/out: a copy, the caller's stay
        chal = _out(count * nchal * FR)
        ver = (ctypes.c_int * max(count, 1))()
        self._check(fn(self._h, count, n, *[_in(b) for b in points + scalars], _in(proofs), _in(rand), st, chal if challenges else None, ver))
        from .whisk import SerializationError
        marks = {CPX_OK: lambda i: True, CPX_ERR_VERIFY: lambda i: False, CPX_ERR_DESERIALIZE: lambda i: SerializationError("%s: proof %d" % (name, i))}
        out = dict(verdicts=[marks[ver[i]](i) for i in range(count)], states=bytes(st)[:count * TRANSCRIPT_BYTES])
        if challenges:
            out["challenges"] = bytes(chal)[:count * nchal * FR]
        return out

    def ipa_verify(self, n, G, crs_H, C, D, z, vec_u, proofs, rand, states, challenges=False):
        """InnerProductProof::verify (inner_product_argument.rs:202-326) for len(z) // 32 independent stand-alone proofs of n elements in ONE
        call (cpx_ipa_verify), each against an accumulator of its own.  G: the affine bases, item after item; crs_H, C, D: 144-byte Jacobian
        points; z, vec_u: Montgomery limbs; proofs: the reference's `serialize` bytes; rand: two non-zero random factors per item;
        states: the 216-byte transcript states before `verify`.  Returns a dict: "verdicts" (per item True, False or a whisk.SerializationError INSTANCE),
        "states" (advanced by the whole verify; unchanged for an item that does not deserialise), and with challenges=True "challenges"
        (per item alpha, beta, gamma_1..L)."""
        count = len(z) // FR
        L = max(n.bit_length() - 1, 0)
        if len(z) != count * FR or len(G) != count * n * AFF or len(vec_u) != count * n * FR or any(len(p) != count * JAC for p in (crs_H, C, D)):
            raise ValueError("ipa_verify: per item n points in G, n scalars in vec_u, one scalar z and one Jacobian point in crs_H, C and D")
        return self._subarg_verify(self._L.cpx_ipa_verify, "ipa_verify", count, n, (G, crs_H, C, D), (z, vec_u), proofs, rand, states, 2, 2 + L,
                                   48 * (2 + 4 * L) + 64, challenges)

    def same_msm_verify(self, n, G, T, U, A, Z_t, Z_u, proofs, rand, states, challenges=False):
        """SameMultiscalarProof::verify (same_multiscalar_argument.rs:153-261) likewise (cpx_same_msm_verify), len(A) // 144 items: three
        random factors per item; "challenges" holds alpha, gamma_1..L."""
        count = len(A) // JAC
        L = max(n.bit_length() - 1, 0)
        if any(len(p) != count * JAC for p in (A, Z_t, Z_u)) or any(len(v) != count * n * AFF for v in (G, T, U)):
            raise ValueError("same_msm_verify: per item n points in G, T and U and one Jacobian point in A, Z_t and Z_u")
        return self._subarg_verify(self._L.cpx_same_msm_verify, "same_msm_verify", count, n, (G, T, U, A, Z_t, Z_u), (), proofs, rand, states, 3, 1 + L,
                                   48 * (3 + 6 * L) + 32, challenges)

    def _subarg_prove(self, fns, name, count, n, inputs, draws_each, states, rand, rngs, nchal, proof_bytes, challenges):
        if n < 0:
            raise ValueError("n is not negative")
        if (rand is None) == (rngs is None):
            raise ValueError("%s: exactly one of rand and rngs" % name)
        if len(states) != count * TRANSCRIPT_BYTES:
            raise ValueError("%s: one 216-byte transcript state per item" % name)
        st = (ctypes.c_uint8 * max(len(states), 1)).from_buffer_copy(bytes(states) if count else b"\0")   # in/out: a copy, the caller's stay
        proofs, chal = _out(count * proof_bytes), _out(count * nchal * FR)
        status = (ctypes.c_int * max(count, 1))(*([CPX_ERR_INTERNAL] * max(count, 1)))   # an entry the library does not write is never read as a proof
        tail = (st, proofs, chal if challenges else None, status)
        if rngs is not None:
            from . import rng as _rng
            if len(rngs) != count:
                raise ValueError("%s: one rng per item" % name)
            if len({r.state for r in rngs}) != count:
                raise ValueError("rngs: identical states draw identical blinders; derive the streams with StdRng.split")
            rs = _rng.load_states(rngs)
            self._check(fns[1](self._h, count, n, *[_in(b) for b in inputs], rs, *tail))
            _rng.store_states(rngs, rs)
        else:
            if len(rand) != count * max(draws_each, 0) * FR:
                raise ValueError("%s: %d draws per item" % (name, draws_each))
            self._check(fns[0](self._h, count, n, *[_in(b) for b in inputs], _in(rand), *tail))
        marks = {CPX_OK: lambda i: True, CPX_ERR_ARG: lambda i: ValueError("%s: item %d has no blinders (the reference panics in generate_ipa_blinders)" % (name, i))}
        out = dict(proofs=[bytes(proofs)[proof_bytes * i:proof_bytes * (i + 1)] for i in range(count)], states=bytes(st)[:count * TRANSCRIPT_BYTES],
                   status=[marks[status[i]](i) for i in range(count)])
        if challenges:
            out["challenges"] = bytes(chal)[:count * nchal * FR]
        if rngs is not None:
            out["rngs"] = b"".join(r.state for r in rngs)
        return out

    def ipa_prove(self, n, G, G_prime, crs_H, C, D, z, vec_c, vec_d, states, rand=None, rngs=None, challenges=False):
        """InnerProductProof::new (inner_product_argument.rs:98-199) for len(z) // 32 independent stand-alone statements of n elements in ONE
        call (cpx_ipa_prove / cpx_ipa_prove_rng).  G, G_prime: the affine bases, item after item; crs_H, C, D: 144-byte Jacobian points;
        z, vec_c, vec_d: Montgomery limbs; states: the 216-byte transcript states before `new`.  Exactly one of rand (per item the 2 n - 2
        draws of generate_ipa_blinders: r, then z) and rngs (one curdleproofs_amd.rng.StdRng per item, DISTINCT streams: the draws are made
        on the device and every stream advances).  Returns a dict: "proofs" (per item the reference's `serialize` bytes, what ipa_verify
        takes), "states" (advanced by the whole `new`), "status" (per item True, or a ValueError INSTANCE where the reference panics in
        generate_ipa_blinders: that item's proof is zero bytes and its state unchanged), with challenges=True "challenges" (per item alpha,
        beta, gamma_1..L), and with rngs "rngs" (the advanced 40-byte states, as the StdRng objects now hold them)."""
        count = len(z) // FR
        L = max(n.bit_length() - 1, 0)
        if len(z) != count * FR or any(len(v) != count * n * AFF for v in (G, G_prime)) or any(len(v) != count * n * FR for v in (vec_c, vec_d)) or \
                any(len(p) != count * JAC for p in (crs_H, C, D)):
            raise ValueError("ipa_prove: per item n points in G and G_prime, n scalars in vec_c and vec_d, one scalar z and one Jacobian point in crs_H, C and D")
        return self._subarg_prove((self._L.cpx_ipa_prove, self._L.cpx_ipa_prove_rng), "ipa_prove", count, n, (G, G_prime, crs_H, C, D, z, vec_c, vec_d), 2 * n - 2,
                                  states, rand, rngs, 2 + L, 48 * (2 + 4 * L) + 64, challenges)

    def same_msm_prove(self, n, G, T, U, A, Z_t, Z_u, vec_x, states, rand=None, rngs=None, challenges=False):
        """SameMultiscalarProof::new (same_multiscalar_argument.rs:69-150) likewise (cpx_same_msm_prove / cpx_same_msm_prove_rng), len(A) // 144
        items: rand is vec_r, n draws per item; "challenges" holds alpha, gamma_1..L; every status is True."""
        count = len(A) // JAC
        L = max(n.bit_length() - 1, 0)
        if any(len(p) != count * JAC for p in (A, Z_t, Z_u)) or any(len(v) != count * n * AFF for v in (G, T, U)) or len(vec_x) != count * n * FR:
            raise ValueError("same_msm_prove: per item n points in G, T and U, n scalars in vec_x and one Jacobian point in A, Z_t and Z_u")
        return self._subarg_prove((self._L.cpx_same_msm_prove, self._L.cpx_same_msm_prove_rng), "same_msm_prove", count, n, (G, T, U, A, Z_t, Z_u, vec_x), n,
                                  states, rand, rngs, 1 + L, 48 * (3 + 6 * L) + 32, challenges)

    def gprod_prove(self, ell, G, H, crs_U, B, gprod_result, vec_b, vec_b_blinders, states, rand=None, rngs=None, challenges=False):
        """GrandProductProof::new (grand_product_argument.rs:43-166) for len(gprod_result) // 32 independent stand-alone statements of ell
        factors each in ONE call (cpx_gprod_prove / cpx_gprod_prove_rng); n_blinders is what vec_b_blinders holds per item, and
        n = ell + n_blinders a power of two.  G (ell per item), H (n_blinders per item): the affine bases, item after item; crs_U, B:
        144-byte Jacobian points; gprod_result, vec_b, vec_b_blinders: Montgomery limbs; states: the 216-byte transcript states before
        `new`.  Exactly one of rand (per item vec_c_blinders, then the 2 n - 2 draws of generate_ipa_blinders) and rngs (as ipa_prove).
        Returns the dict of ipa_prove: "proofs" are C, r_p and the InnerProductProof bytes, "challenges" per item gprod alpha, gprod beta,
        ipa alpha, ipa beta, gamma_1..L."""
        count = len(gprod_result) // FR
        nb = len(vec_b_blinders) // (count * FR) if count else 0
        n = ell + nb
        L = max(n.bit_length() - 1, 0)
        if len(gprod_result) != count * FR or len(G) != count * ell * AFF or len(H) != count * nb * AFF or len(vec_b) != count * ell * FR or \
                len(vec_b_blinders) != count * nb * FR or any(len(p) != count * JAC for p in (crs_U, B)):
            raise ValueError("gprod_prove: per item ell points in G and scalars in vec_b, n_blinders points in H and scalars in vec_b_blinders, one scalar "
                             "gprod_result and one Jacobian point in crs_U and B")
        fns = tuple((lambda h, cnt, _n, *rest, fn=fn: fn(h, cnt, ell, nb, *rest)) for fn in (self._L.cpx_gprod_prove, self._L.cpx_gprod_prove_rng))
        return self._subarg_prove(fns, "gprod_prove", count, n, (G, H, crs_U, B, gprod_result, vec_b, vec_b_blinders), nb + 2 * n - 2, states, rand, rngs, 4 + L,
                                  48 * (3 + 4 * L) + 96, challenges)

    def gprod_verify(self, ell, G, H, crs_U, crs_G_sum, crs_H_sum, B, gprod_result, proofs, rand, states, challenges=False):
        """GrandProductProof::verify (grand_product_argument.rs:180-246) for len(gprod_result) // 32 independent stand-alone proofs of ell
        factors in ONE call (cpx_gprod_verify); n_blinders is what H holds per item.  crs_G_sum, crs_H_sum: the affine sums, taken from
        the caller as in the reference; proofs: what gprod_prove returns; rand: two non-zero factors per item.  Returns the dict of
        ipa_verify; "challenges" per item gprod alpha, gprod beta, ipa alpha, ipa beta, gamma_1..L."""
        count = len(gprod_result) // FR
        nb = len(H) // (count * AFF) if count else 0
        n = ell + nb
        L = max(n.bit_length() - 1, 0)
        if len(gprod_result) != count * FR or len(G) != count * ell * AFF or len(H) != count * nb * AFF or any(len(p) != count * JAC for p in (crs_U, B)) or \
                any(len(p) != count * AFF for p in (crs_G_sum, crs_H_sum)):
            raise ValueError("gprod_verify: per item ell points in G, n_blinders points in H, one scalar gprod_result, one Jacobian point in crs_U and B and one "
                             "affine point in crs_G_sum and crs_H_sum")
        fn = lambda h, cnt, _n, *rest: self._L.cpx_gprod_verify(h, cnt, ell, nb, *rest)
        return self._subarg_verify(fn, "gprod_verify", count, n, (G, H, crs_U, crs_G_sum, crs_H_sum, B), (gprod_result,), proofs, rand, states, 2, 4 + L,
                                   48 * (3 + 4 * L) + 96, challenges)

    def same_perm_prove(self, ell, G, H, crs_U, A, M, vec_a, permutation, vec_a_blinders, vec_m_blinders, states, rand=None, rngs=None, challenges=False):
        """SamePermutationProof::new (same_permutation_argument.rs:40-99) for len(A) // 144 independent stand-alone statements of ell
        elements each in ONE call (cpx_same_perm_prove / cpx_same_perm_prove_rng); n_blinders is what vec_a_blinders holds per item, and
        n = ell + n_blinders a power of two.  G (ell per item), H (n_blinders per item): the affine bases, item after item; crs_U, A, M:
        144-byte Jacobian points; vec_a, vec_a_blinders, vec_m_blinders: Montgomery limbs; permutation: ell values below ell per item,
        a sequence of integers or their little-endian u32 bytes; states: the 216-byte transcript states before `new`.  Exactly one of
        rand (the draws of gprod_prove: this layer draws nothing) and rngs (as ipa_prove).  Returns the dict of gprod_prove: "proofs" are B
        and the GrandProductProof bytes, "challenges" per item same-perm alpha, beta, then those of gprod_prove."""
        import struct
        count = len(A) // JAC
        if not isinstance(permutation, (bytes, bytearray, memoryview)):
            permutation = list(permutation)
            if any(not 0 <= int(v) < 1 << 32 for v in permutation):
                raise ValueError("same_perm_prove: the permutation's entries are u32 values")
            permutation = struct.pack("<%dI" % len(permutation), *permutation)
        nb = len(vec_a_blinders) // (count * FR) if count else 0
        n = ell + nb
        L = max(n.bit_length() - 1, 0)
        if len(G) != count * ell * AFF or len(H) != count * nb * AFF or len(vec_a) != count * ell * FR or len(permutation) != count * ell * 4 or \
                any(len(v) != count * nb * FR for v in (vec_a_blinders, vec_m_blinders)) or any(len(p) != count * JAC for p in (crs_U, A, M)):
            raise ValueError("same_perm_prove: per item ell points in G, scalars in vec_a and entries in permutation, n_blinders points in H and scalars in "
                             "vec_a_blinders and vec_m_blinders, and one Jacobian point in crs_U, A and M")
        fns = tuple((lambda h, cnt, _n, *rest, fn=fn: fn(h, cnt, ell, nb, *rest)) for fn in (self._L.cpx_same_perm_prove, self._L.cpx_same_perm_prove_rng))
        return self._subarg_prove(fns, "same_perm_prove", count, n, (G, H, crs_U, A, M, vec_a, permutation, vec_a_blinders, vec_m_blinders), nb + 2 * n - 2, states,
                                  rand, rngs, 6 + L, 48 * (4 + 4 * L) + 96, challenges)

    def same_perm_verify(self, ell, G, H, crs_U, crs_G_sum, crs_H_sum, A, M, vec_a, proofs, rand, states, challenges=False):
        """SamePermutationProof::verify (same_permutation_argument.rs:112-171) for len(A) // 144 independent stand-alone proofs of ell
        elements in ONE call (cpx_same_perm_verify); n_blinders is what H holds per item.  crs_G_sum, crs_H_sum: the affine sums, taken
        from the caller as in the reference; proofs: what same_perm_prove returns; rand: THREE non-zero factors per item, the
        same-permutation check's first.  Returns the dict of gprod_verify; "challenges" per item same-perm alpha, beta, then those of
        gprod_verify."""
        count = len(A) // JAC
        nb = len(H) // (count * AFF) if count else 0
        n = ell + nb
        L = max(n.bit_length() - 1, 0)
        if len(G) != count * ell * AFF or len(H) != count * nb * AFF or len(vec_a) != count * ell * FR or any(len(p) != count * JAC for p in (crs_U, A, M)) or \
                any(len(p) != count * AFF for p in (crs_G_sum, crs_H_sum)):
            raise ValueError("same_perm_verify: per item ell points in G and scalars in vec_a, n_blinders points in H, one Jacobian point in crs_U, A and M and "
                             "one affine point in crs_G_sum and crs_H_sum")
        fn = lambda h, cnt, _n, *rest: self._L.cpx_same_perm_verify(h, cnt, ell, nb, *rest)
        return self._subarg_verify(fn, "same_perm_verify", count, n, (G, H, crs_U, crs_G_sum, crs_H_sum, A, M), (vec_a,), proofs, rand, states, 3, 6 + L,
                                   48 * (4 + 4 * L) + 96, challenges)

    def normalize(self, jac, compressed=False):
        n = len(jac) // JAC
        a, c = _out(AFF * n), _out(48 * n)
        self._check(self._L.cpx_g1_normalize(self._h, _in(jac), n, a, c))
        return (bytes(a)[: AFF * n], bytes(c)[: 48 * n]) if compressed else bytes(a)[: AFF * n]

    def decompress(self, comp, check_subgroup=True):
        n = len(comp) // 48
        o = _out(AFF * n)
        self._check(self._L.cpx_g1_decompress(self._h, _in(comp), n, o, 1 if check_subgroup else 0))
        return bytes(o)[: AFF * n]

    def clear_cofactor(self, points):
        """[h] P for every point of `points` — ANY points of E(Fp), 96 bytes each — with the full cofactor h = |E(Fp)| / r (ark-ec
        `mul_by_cofactor`; cpx_g1_clear_cofactor: a compiled-in addition chain, whatever option scale_any_point says).  Returns the affine
        points, the identity as 96 zero bytes."""
        n = len(points) // AFF
        if len(points) % AFF:
            raise ValueError("clear_cofactor: 96 bytes per affine point")
        o = _out(AFF * n)
        self._check(self._L.cpx_g1_clear_cofactor(self._h, _in(points), n, o))
        return bytes(o)[: AFF * n]

    def generator_mul(self, scalars, compressed=False):
        """scalars[i] * G for the G1 generator, count per call on the generator's fixed-base table (cpx_g1_generator_mul; whisk.rs:318,323
        with g1 = generator).  scalars: count wire scalars back to back.  Returns the affine points, or (affine, compressed)."""
        n = len(scalars) // FR
        if len(scalars) % FR:
            raise ValueError("generator_mul: 32 bytes per scalar")
        a, c = _out(AFF * n), _out(48 * n)
        self._check(self._L.cpx_g1_generator_mul(self._h, n, _in(scalars), a, c if compressed else None))
        return (bytes(a)[: AFF * n], bytes(c)[: 48 * n]) if compressed else bytes(a)[: AFF * n]

    def decompress_status(self, comp, check_subgroup=True):
        """per-point form: (affine points, list of status bytes: 0 ok, 1 malformed / not on the curve, 2 not in the subgroup)"""
        n = len(comp) // 48
        o, st = _out(AFF * n), _out(n)
        self._check(self._L.cpx_g1_decompress_status(self._h, _in(comp), n, o, 1 if check_subgroup else 0, st))
        return bytes(o)[: AFF * n], list(bytes(st)[:n])

    # ---- tier 2 ----
    def load_batch(self, vec_R, vec_S, vec_T, vec_U, M):
        """Uploads `batch` instances (concatenated per-proof buffers)."""
        if self.ell is None:
            raise CpxError(CPX_ERR_STATE, "set_crs first")
        batch = len(M) // JAC
        if batch == 0 or len(M) % JAC:
            raise ValueError("M: one Jacobian point (144 bytes) per instance")
        for v in (vec_R, vec_S, vec_T, vec_U):
            if len(v) != batch * self.ell * AFF:
                raise ValueError("every instance vector must hold batch * ell affine points (%d bytes), got %d" % (batch * self.ell * AFF, len(v)))
        self._check(self._L.cpx_batch_load(self._h, batch, _in(vec_R), _in(vec_S), _in(vec_T), _in(vec_U), _in(M)))

    def load_batch_begin(self, vec_R, vec_S, vec_T, vec_U, M):
        """Starts uploading the NEXT batch beside the kernels of the loaded one (cpx_batch_load_begin); the buffers — best page-locked ones from
        `marshal` — must stay untouched until load_batch_end() returns, which makes the staged batch the loaded one."""
        if self.ell is None:
            raise CpxError(CPX_ERR_STATE, "set_crs first")
        batch = len(M) // JAC
        if batch == 0 or len(M) % JAC:
            raise ValueError("M: one Jacobian point (144 bytes) per instance")
        for v in (vec_R, vec_S, vec_T, vec_U):
            if len(v) != batch * self.ell * AFF:
                raise ValueError("every instance vector must hold batch * ell affine points (%d bytes), got %d" % (batch * self.ell * AFF, len(v)))
        self._staged = tuple(_in(v) for v in (vec_R, vec_S, vec_T, vec_U, M))   # kept alive until load_batch_end
        self._check(self._L.cpx_batch_load_begin(self._h, batch, *self._staged))

    def load_batch_end(self):
        try:
            self._check(self._L.cpx_batch_load_end(self._h))
        finally:
            self._staged = None

    @staticmethod
    def marshal(data):
        """Pre-marshal a bytes object (or a list of u32 for permutations) into a page-locked ctypes buffer once (cpx_host_alloc), so
        that repeated batch calls pay neither Python-side copies nor staging copies: the library moves it by asynchronous DMA."""
        if isinstance(data, (bytes, bytearray)):
            buf = _pinned_array(ctypes.c_uint8, max(len(data), 1))
            ctypes.memmove(buf, bytes(data) if len(data) else b"\0", max(len(data), 1))
            return buf
        buf = _pinned_array(ctypes.c_uint32, max(len(data), 1))
        buf[:len(data)] = data
        return buf

    def prove_batch(self, permutations, k, vec_m_blinders, rand, raw=False):
        """CurdleproofsProof::new for every loaded instance; returns a list of serialized proofs (or, with raw=True, a page-locked
        ctypes buffer holding all of them back to back; it is reused by the second-next raw prove of this context)."""
        B, ell, n = self.batch, self.ell, self.n
        if not isinstance(permutations, ctypes.Array):
            if len(permutations) != B * ell:
                raise ValueError("permutations: batch * ell entries")
            permutations = (ctypes.c_uint32 * (B * ell))(*permutations)
        perm = permutations
        if ctypes.sizeof(perm) != 4 * B * ell or _len(k) != B * FR or _len(vec_m_blinders) != B * 4 * FR or _len(rand) != B * (3 * n + 9) * FR:
            raise ValueError("prove_batch: per instance ell u32 permutation entries, k (32 B), 4 blinders, 3n+9 random scalars")
        psz = self.proof_size
        if raw:   # two page-locked output buffers per context, used alternately: a returned buffer stays valid until the prove after the next
            pool = self.__dict__.setdefault("_raw_pool", {})
            slot = pool.get("next", 0)
            if pool.get(("size", slot)) != B * psz:
                pool[("buf", slot)] = _pinned_array(ctypes.c_uint8, B * psz)
                pool[("size", slot)] = B * psz
            out = pool[("buf", slot)]
            pool["next"] = 1 - slot
        else:
            out = _out(B * psz)
        self._check(self._L.cpx_batch_prove(self._h, perm, _in(k), _in(vec_m_blinders), _in(rand), out))
        if raw:
            return out
        blob = bytes(out)
        return [blob[i * psz:(i + 1) * psz] for i in range(B)]

    def verify_batch(self, proofs, rand):
        """CurdleproofsProof::verify for every loaded instance; returns a list of CPX_* verdicts.
        `proofs`: list of serialized proofs, or the raw buffer prove_batch(raw=True) returned."""
        B = self.batch
        psz = self.proof_size
        blob = proofs if isinstance(proofs, ctypes.Array) else b"".join(proofs)
        if _len(blob) != B * psz or _len(rand) != B * 8 * FR:
            raise ValueError("verify_batch: batch * proof_size proof bytes and 8 random factors per proof")
        verdict = (ctypes.c_int * B)(*([CPX_ERR_INTERNAL] * B))   # an entry the library does not write is never read as "accepted"
        self._check(self._L.cpx_batch_verify(self._h, _in(blob), _in(rand), verdict))
        return list(verdict)

    def verify_batch_grouped(self, proofs, rand):
        """CurdleproofsProof::verify for every loaded instance through the grouped form of the accumulated check
        (cpx_batch_verify_grouped): the batch is cut into at most `locate_groups_max` groups, every group's accumulated sum is tested,
        and only the proofs of a failing group get a check of their own.  `rand`: 12 Fr per proof, as for verify_batch_fused.
        Returns (list of CPX_* verdicts, n_rechecked)."""
        B = self.batch
        psz = self.proof_size
        blob = proofs if isinstance(proofs, ctypes.Array) else b"".join(proofs)
        if _len(blob) != B * psz or _len(rand) != B * 12 * FR:
            raise ValueError("verify_batch_grouped: batch * proof_size proof bytes and 12 random factors per proof")
        verdict = (ctypes.c_int * max(B, 1))(*([CPX_ERR_INTERNAL] * max(B, 1)))   # an entry the library does not write is never read as "accepted"
        rechecked = ctypes.c_size_t(0)
        self._check(self._L.cpx_batch_verify_grouped(self._h, _in(blob), _in(rand), verdict, ctypes.byref(rechecked)))
        return list(verdict)[:B], rechecked.value

    def shuffle_batch(self, vec_R, vec_S, permutations, k, vec_m_blinders):
        """util.rs:83-106 for every instance in ONE library call (cpx_batch_shuffle): vec_R / vec_S hold count * ell affine points,
        permutations count * ell entries, k count scalars, vec_m_blinders 4 per instance.  Returns (vec_T, vec_U, M) — affine, affine,
        Jacobian, concatenated per instance — and leaves the count instances loaded (self.batch == count)."""
        if self.ell is None:
            raise CpxError(CPX_ERR_STATE, "set_crs first")
        ell = self.ell
        count = _len(k) // FR
        if not isinstance(permutations, ctypes.Array):
            if len(permutations) != count * ell:
                raise ValueError("permutations: count * ell entries")
            permutations = (ctypes.c_uint32 * max(count * ell, 1))(*permutations)
        if (_len(k) != count * FR or _len(vec_R) != count * ell * AFF or _len(vec_S) != count * ell * AFF or _len(vec_m_blinders) != count * N_BLINDERS * FR
                or ctypes.sizeof(permutations) != 4 * max(count * ell, 1)):
            raise ValueError("shuffle_batch: per instance ell affine points in vec_R and vec_S, ell u32 permutation entries, k (32 B), 4 blinders")
        if count == 0:
            return b"", b"", b""
        t, u, m = _out(count * ell * AFF), _out(count * ell * AFF), _out(count * JAC)
        self._check(self._L.cpx_batch_shuffle(self._h, count, _in(vec_R), _in(vec_S), permutations, _in(k), _in(vec_m_blinders), t, u, m))
        return bytes(t), bytes(u), bytes(m)

    # ---- measurement ----
    def verify_batch_fused_partial(self, proofs, rand):
        """BASELINE config 5: one accumulated MSM over all loaded proofs.  `rand`: 12 Fr per proof.
        Returns (partial sum as a 144-byte Jacobian point, number of structurally invalid proofs)."""
        data = proofs if isinstance(proofs, (bytes, bytearray)) or hasattr(proofs, "_length_") else b"".join(proofs)
        if _len(data) != self.batch * self.proof_size or _len(rand) != self.batch * 12 * FR:
            raise ValueError("verify_batch_fused: batch * proof_size proof bytes and 12 random factors per proof")
        out = _out(JAC)
        bad = ctypes.c_int(0)
        self._check(self._L.cpx_batch_verify_fused(self._h, _in(data), _in(rand), out, ctypes.byref(bad)))
        return bytes(out)[:JAC], bad.value

    def sum_jac(self, points_jac):
        """sum of Jacobian points -> (sum, is_identity)"""
        n = len(points_jac) // JAC
        if len(points_jac) % JAC:
            raise ValueError("sum_jac: 144 bytes per point")
        out = _out(JAC)
        flag = ctypes.c_int(0)
        self._check(self._L.cpx_g1_sum_jac(self._h, _in(points_jac), n, out, ctypes.byref(flag)))
        return bytes(out)[:JAC], bool(flag.value)

    def verify_batch_fused(self, proofs, rand):
        """Single-context form of config 5: True iff every loaded proof is valid (all-or-nothing)."""
        part, bad = self.verify_batch_fused_partial(proofs, rand)
        return bad == 0 and self.sum_jac(part)[1]

    def set_profiling(self, on=True):
        self._check(self._L.cpx_set_profiling(self._h, 1 if on else 0))

    def reset_stats(self):
        self._check(self._L.cpx_reset_stats(self._h))

    def stat(self, name):
        n, ms, by, un = ctypes.c_uint64(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._L.cpx_get_stat(self._h, name.encode(), ctypes.byref(n), ctypes.byref(ms), ctypes.byref(by), ctypes.byref(un)))
        return dict(launches=n.value, ms=ms.value, alg_bytes=by.value, units=un.value)

    KERNELS = ("k_msm_tblw<32, false>", "k_reduce_sets", "k_msm_tblw<16, false>", "k_msm_tblw<8, false>", "k_msm_tblw<4, false>", "k_msm_tblw<2, false>", "k_msm_fix<19, 7>", "k_msm_fix<16, 4>", "k_msm_fix<16, 2>", "k_msm_fix<16, 16>", "k_msm_fix<16, 8>", "k_msm_fix<8, 16>", "k_msm_fix<8, 8>",
               "k_transcript_step1", "k_msm_tblw_pair", "k_late_fix", "k_late_uniform", "k_late_tables", "k_late_msm", "k_finalize_ranges", "k_table_build", "k_msm_accw", "k_msm_tblw<2, true>", "k_msm_tail", "k_smul", "k_finalize", "k_compress", "k_decompress", "k_tracker_challenge", "k_tracker_relations", "k_shuffle_status", "k_shuffle_gather", "k_shuffle_commit", "k_run_gather", "k_run_commit", "k_gen_table", "k_gen_mul", "k_fix_build", "k_find_scan", "k_find_compare", "k_tracker_check_scalars", "k_tracker_gather", "k_vs_crs_sum_groups", "k_rng_draw", "k_rng_g1_scan", "k_rng_g1_sqrt", "k_rng_g1_select", "k_clear_cofactor", "k_subarg_scalars", "k_loop_step", "k_smul_quad", "k_subarg_blinders", "k_subarg_prove_setup", "k_gprod_products", "k_gprod_setup", "k_gprod_rdu", "k_gprod_verify_steps", "k_same_perm_step", "k_same_perm_verify_step", "k_same_perm_weights", "host_parallel_for", "host_wait_device", "host_prove_wall", "host_verify_wall")

    def stats(self):
        return {k: self.stat(k) for k in self.KERNELS}

    def set_host_threads(self, t):
        self._check(self._L.cpx_set_host_threads(self._h, t))

    def bench_fpmul(self, blocks=2048, iters=2000, reps=3):
        r = ctypes.c_double(0)
        self._check(self._L.cpx_bench_fpmul(self._h, blocks, iters, reps, ctypes.byref(r)))
        return r.value


class MsmAccumulator:
    """msm_accumulator.rs:22-68.  The random factor is drawn by the caller (the RNG stays outside)."""

    def __init__(self, ctx):
        self._ctx = ctx
        self._L = ctx._L
        h = ctypes.c_void_p()
        ctx._check(self._L.cpx_accum_new(ctx._h, ctypes.byref(h)))
        self._h = h

    def accumulate_check(self, C, vec_x, vec_V, random_factor):
        n = min(len(vec_x) // FR, len(vec_V) // AFF)   # Rust `zip`
        self._ctx._check(self._L.cpx_accum_check(self._h, _in(C), _in(vec_x), _in(vec_V), n, _in(random_factor)))

    def verify(self):
        rc = self._L.cpx_accum_verify(self._h)
        if rc == CPX_ERR_VERIFY:
            raise ProofError(rc)
        self._ctx._check(rc)

    def __del__(self):
        try:
            if self._h:
                self._L.cpx_accum_free(self._h)
                self._h = None
        except Exception:
            pass


class CurdleproofsProof:
    """One serialized proof, with the reference's constructor / verifier names (curdleproofs.rs:59,197)."""

    def __init__(self, data):
        self.data = bytes(data)

    @staticmethod
    def new(ctx, vec_R, vec_S, vec_T, vec_U, M, permutation, k, vec_m_blinders, rand):
        ctx.load_batch(vec_R, vec_S, vec_T, vec_U, M)
        return CurdleproofsProof(ctx.prove_batch(list(permutation), k, vec_m_blinders, rand)[0])

    def verify(self, ctx, vec_R, vec_S, vec_T, vec_U, M, rand):
        ctx.load_batch(vec_R, vec_S, vec_T, vec_U, M)
        v = ctx.verify_batch([self.data], rand)[0]
        if v == CPX_ERR_VERIFY:
            raise ProofError(v)
        if v != CPX_OK:
            raise CpxError(v)

    def serialize(self):
        return self.data

    @staticmethod
    def deserialize(data, log2_n):
        if len(data) != 48 * (18 + 10 * log2_n) + 32 * 7:
            raise CpxError(CPX_ERR_DESERIALIZE, "wrong length")
        return CurdleproofsProof(data)
