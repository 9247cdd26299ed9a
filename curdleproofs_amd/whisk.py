"""Byte-level Whisk API: host-side mirror of the reference's `src/whisk.rs` on top of the C-ABI (`cpx_whisk_*`).

Same function names and argument meaning as the Rust `pub fn`s; a tracker is the pair of 48-byte compressed points
`(r_G, k_r_G)` (`WhiskTracker`, whisk.rs:36-42).  Everything that touches the group runs on the GPU through `Context`;
there is no CPU path.  The reference threads an `rng` through these functions; here the RNG stays with the caller
(SURVEY 8b): each function takes the values the reference would have drawn, in the reference's order, or — when they
are omitted — draws them from the OS CSPRNG (`secrets`), which is what a production caller wants.
"""
import ctypes
import secrets

from . import AFF, FR, CPX_ERR_DESERIALIZE, CPX_ERR_INTERNAL, CPX_ERR_VERIFY, CPX_NO_OWNER, CPX_OK, CpxError, _in, _out   # noqa: F401
from . import params as pr

FIELD_ELEMENT_SIZE = 32        # whisk.rs:21
G1POINT_SIZE = 48              # whisk.rs:22
TRACKER_PROOF_SIZE = 128       # whisk.rs:25
N_BLINDERS = 4


class SerializationError(CpxError):
    """ark_serialize::SerializationError of the reference's `Result`s."""

    def __init__(self, detail=""):
        super().__init__(CPX_ERR_DESERIALIZE, detail)


class WhiskTracker:
    """whisk.rs:36-42"""

    def __init__(self, r_G, k_r_G):
        if len(r_G) != G1POINT_SIZE or len(k_r_G) != G1POINT_SIZE:
            raise ValueError("a tracker is two 48-byte compressed G1 points")
        self.r_G, self.k_r_G = bytes(r_G), bytes(k_r_G)

    def to_bytes(self):
        return self.r_G + self.k_r_G

    def __eq__(self, other):
        return isinstance(other, WhiskTracker) and self.to_bytes() == other.to_bytes()

    @staticmethod
    def from_k_r(ctx, k, r):
        """whisk.rs:45-55: r_G = r * G, k_r_G = k * r_G (k, r: 32-byte wire scalars)"""
        r_G = bls_g1_scalar_multiply(ctx, g1_generator(ctx), r)
        k_r_G = bls_g1_scalar_multiply(ctx, r_G, k)
        return WhiskTracker(to_bytes_g1affine(ctx, r_G), to_bytes_g1affine(ctx, k_r_G))


def _cat(trackers):
    return b"".join(t.to_bytes() for t in trackers)


def _check(ctx, rc):
    if rc == CPX_ERR_DESERIALIZE:
        raise SerializationError(ctx._L.cpx_last_error(ctx._h).decode(errors="replace"))
    ctx._check(rc)


def _rand_fr(n):
    return pr.random_fr_wire(None, n)


def whisk_shuffle_proof_size(ctx):
    """WHISK_SHUFFLE_PROOF_SIZE (whisk.rs:23: 4496 at the reference's fixed ell = 124) for the CRS loaded into ctx"""
    return G1POINT_SIZE + ctx.proof_size


def generate_whisk_shuffle_proof(ctx, pre_trackers, permutation=None, k=None, vec_m_blinders=None, rand=None, rng=None):
    """whisk.rs:144-179.  Returns (post_trackers, whisk_shuffle_proof_bytes).  ctx must hold the CRS (`Context.set_crs`).
    permutation / k / vec_m_blinders / rand are the reference's rng draws (shuffle of 0..ell, Fr::rand, 4 blinders, the
    3n+9 draws of CurdleproofsProof::new); omitted values come from the OS CSPRNG.
    rng (a curdleproofs_amd.rng.StdRng, instead of the four): the draws are made on the device from its state, in the reference's order,
    and rng advances as the crate's would — by the shuffle and k only when a pre tracker does not decode (whisk.rs:150-157)."""
    ell, n = ctx.ell, ctx.n
    if len(pre_trackers) != ell:
        raise ValueError("need exactly ell = %d trackers" % ell)
    if rng is not None:
        if not (permutation is None and k is None and vec_m_blinders is None and rand is None):
            raise ValueError("either rng or explicit draws")
        res = generate_whisk_shuffle_proofs(ctx, [pre_trackers], rngs=[rng])[0]
        if res is None:
            raise SerializationError("undecodable pre tracker")
        return res
    if permutation is None:
        permutation = list(range(ell))
        for i in range(ell - 1, 0, -1):                      # Fisher-Yates on the CSPRNG
            j = secrets.randbelow(i + 1)
            permutation[i], permutation[j] = permutation[j], permutation[i]
    k = _rand_fr(1) if k is None else k
    vec_m_blinders = _rand_fr(N_BLINDERS) if vec_m_blinders is None else vec_m_blinders
    rand = _rand_fr(3 * n + 9) if rand is None else rand
    if len(permutation) != ell or len(k) != FR or len(vec_m_blinders) != N_BLINDERS * FR or len(rand) != (3 * n + 9) * FR:
        raise ValueError("bad argument lengths")
    post, proof = _out(ell * 2 * G1POINT_SIZE), _out(whisk_shuffle_proof_size(ctx))
    perm = (ctypes.c_uint32 * ell)(*permutation)
    _check(ctx, ctx._L.cpx_whisk_generate_shuffle_proof(ctx._h, _in(_cat(pre_trackers)), perm, _in(k), _in(vec_m_blinders), _in(rand), post, proof))
    pb = bytes(post)
    return [WhiskTracker(pb[96 * i:96 * i + 48], pb[96 * i + 48:96 * i + 96]) for i in range(ell)], bytes(proof)


def is_valid_whisk_shuffle_proof(ctx, pre_trackers, post_trackers, whisk_shuffle_proof_bytes, rand=None):
    """whisk.rs:106-130: True / False, or SerializationError for undecodable trackers / proof bytes.
    rand: the verifier's eight accumulate_check factors (msm_accumulator.rs:44); drawn from the CSPRNG when omitted."""
    ell = ctx.ell
    if len(pre_trackers) != ell or len(post_trackers) != ell:
        raise ValueError("need exactly ell = %d trackers on both sides" % ell)
    if len(whisk_shuffle_proof_bytes) != whisk_shuffle_proof_size(ctx):
        raise SerializationError("wrong proof length")      # a fixed-size array in the reference
    rand = _rand_fr(8) if rand is None else rand
    if len(rand) != 8 * FR:
        raise ValueError("8 random factors")
    valid = ctypes.c_int(0)
    _check(ctx, ctx._L.cpx_whisk_is_valid_shuffle_proof(ctx._h, _in(_cat(pre_trackers)), _in(_cat(post_trackers)), _in(whisk_shuffle_proof_bytes), _in(rand),
                                                        ctypes.byref(valid)))
    return bool(valid.value)


def generate_whisk_tracker_proof(ctx, tracker, k, blinder=None):
    """whisk.rs:228-263: 128-byte proof of knowledge of k with tracker.k_r_G == k * tracker.r_G"""
    blinder = _rand_fr(1) if blinder is None else blinder
    if len(k) != FR or len(blinder) != FR:
        raise ValueError("k and blinder are 32-byte wire scalars")
    out = _out(TRACKER_PROOF_SIZE)
    _check(ctx, ctx._L.cpx_whisk_generate_tracker_proof(ctx._h, _in(tracker.to_bytes()), _in(k), _in(blinder), out))
    return bytes(out)


def is_valid_whisk_tracker_proof(ctx, tracker, k_commitment, tracker_proof):
    """whisk.rs:183-226"""
    if len(k_commitment) != G1POINT_SIZE or len(tracker_proof) != TRACKER_PROOF_SIZE:
        raise SerializationError("wrong length")
    valid = ctypes.c_int(0)
    _check(ctx, ctx._L.cpx_whisk_is_valid_tracker_proof(ctx._h, _in(tracker.to_bytes()), _in(k_commitment), _in(tracker_proof), ctypes.byref(valid)))
    return bool(valid.value)


# ---- many shuffle proofs per call (cpx_whisk_generate_shuffle_proofs / cpx_whisk_verify_shuffle_proofs) ----
def _random_permutation(ell):
    permutation = list(range(ell))
    for i in range(ell - 1, 0, -1):                          # Fisher-Yates on the CSPRNG
        j = secrets.randbelow(i + 1)
        permutation[i], permutation[j] = permutation[j], permutation[i]
    return permutation


def generate_whisk_shuffle_proofs(ctx, pre_tracker_lists, permutations=None, ks=None, vec_m_blinders=None, rands=None, rngs=None):
    """whisk.rs:144-179 for every list of ell pre trackers in ONE library call.  permutations / ks / vec_m_blinders / rands: one entry per
    list, the reference's rng draws as in generate_whisk_shuffle_proof; omitted ones come from the OS CSPRNG.  Returns a list of
    (post_trackers, whisk_shuffle_proof_bytes), with None where a pre tracker does not decode (the reference's SerializationError);
    nothing is raised per item.  The count instances stay loaded in ctx.
    rngs (one curdleproofs_amd.rng.StdRng per list, DISTINCT streams — StdRng.split — instead of the four): every item's draws are made on
    the device from its own stream (cpx_whisk_generate_shuffle_proofs_rng) and every stream advances as the crate's rng would."""
    count = len(pre_tracker_lists)
    if rngs is not None:
        if not (permutations is None and ks is None and vec_m_blinders is None and rands is None):
            raise ValueError("either rngs or explicit draws")
        if len(rngs) != count:
            raise ValueError("one rng per tracker list")
        if len({r.state for r in rngs}) != count:
            raise ValueError("rngs: identical states draw identical witnesses; derive the streams with StdRng.split")
    for name, arg in (("permutation", permutations), ("k", ks), ("blinder set", vec_m_blinders), ("set of draws", rands)):
        if arg is not None and len(arg) != count:
            raise ValueError("one %s per tracker list" % name)
    if count == 0:
        return []
    ell, n = ctx.ell, ctx.n
    if any(len(t) != ell for t in pre_tracker_lists):
        raise ValueError("need exactly ell = %d trackers per list" % ell)
    if rngs is None:
        permutations = [_random_permutation(ell) for _ in range(count)] if permutations is None else permutations
        ks = [_rand_fr(1) for _ in range(count)] if ks is None else ks
        vec_m_blinders = [_rand_fr(N_BLINDERS) for _ in range(count)] if vec_m_blinders is None else vec_m_blinders
        rands = [_rand_fr(3 * n + 9) for _ in range(count)] if rands is None else rands
        if (any(len(p) != ell for p in permutations) or any(len(k) != FR for k in ks) or any(len(b) != N_BLINDERS * FR for b in vec_m_blinders)
                or any(len(r) != (3 * n + 9) * FR for r in rands)):
            raise ValueError("bad argument lengths: ell permutation entries, a 32-byte k, 4 blinders and 3n+9 draws per list")
    rec = whisk_shuffle_proof_size(ctx)
    post, proofs = _out(count * ell * 2 * G1POINT_SIZE), _out(count * rec)
    status = (ctypes.c_int * count)(*([CPX_ERR_INTERNAL] * count))   # an entry the library does not write is never read as a proof
    if rngs is not None:
        from . import rng as _rng
        states = _rng.load_states(rngs)
        ctx._check(ctx._L.cpx_whisk_generate_shuffle_proofs_rng(ctx._h, count, _in(b"".join(_cat(t) for t in pre_tracker_lists)), states, post, proofs, status))
        _rng.store_states(rngs, states)
    else:
        perm = (ctypes.c_uint32 * (count * ell))(*[x for p in permutations for x in p])
        ctx._check(ctx._L.cpx_whisk_generate_shuffle_proofs(ctx._h, count, _in(b"".join(_cat(t) for t in pre_tracker_lists)), perm, _in(b"".join(ks)),
                                                            _in(b"".join(vec_m_blinders)), _in(b"".join(rands)), post, proofs, status))
    pb, fb = bytes(post), bytes(proofs)
    res = []
    for i, st in enumerate(status):
        if st not in (CPX_OK, CPX_ERR_DESERIALIZE):
            raise CpxError(st, "shuffle proof %d" % i)
        if st != CPX_OK:
            res.append(None)
            continue
        row = pb[96 * ell * i:96 * ell * (i + 1)]
        res.append(([WhiskTracker(row[96 * j:96 * j + 48], row[96 * j + 48:96 * j + 96]) for j in range(ell)], fb[rec * i:rec * (i + 1)]))
    return res


def are_valid_whisk_shuffle_proofs(ctx, pre_lists, post_lists, proofs, rands=None):
    """whisk.rs:106-130 for every (pre_trackers, post_trackers, proof) triple in ONE library call.  rands: per triple the verifier's eight
    accumulate_check factors (CSPRNG when omitted).  Returns a list with True / False, or a SerializationError INSTANCE where the reference
    returns Err (undecodable tracker, M or proof bytes, wrong proof length); nothing is raised per item."""
    return _verify_whisk_shuffle_proofs(ctx, pre_lists, post_lists, proofs, rands, 8)[0]


def are_valid_whisk_shuffle_proofs_grouped(ctx, pre_lists, post_lists, proofs, rands=None):
    """The same through the grouped form of the accumulated check (cpx_whisk_verify_shuffle_proofs_grouped): close to the rate of the
    all-or-nothing fused check while few items are wrong.  rands: per triple TWELVE factors (the eight accumulate_check factors, then
    four weights for the SameScalar equalities).  Returns (results as above, n_rechecked): n_rechecked items went through a check of
    their own because the sum of their group was not the identity (context option "locate_groups_max")."""
    return _verify_whisk_shuffle_proofs(ctx, pre_lists, post_lists, proofs, rands, 12)


def _verify_whisk_shuffle_proofs(ctx, pre_lists, post_lists, proofs, rands, nf):
    """nf = 8: cpx_whisk_verify_shuffle_proofs, nf = 12: its grouped form.  Returns (results, n_rechecked)."""
    count = len(pre_lists)
    if len(post_lists) != count or len(proofs) != count or (rands is not None and len(rands) != count):
        raise ValueError("one post tracker list, one proof and one set of factors per pre tracker list")
    if count == 0:
        return [], 0
    ell = ctx.ell
    if any(len(t) != ell for t in pre_lists) or any(len(t) != ell for t in post_lists):
        raise ValueError("need exactly ell = %d trackers per list on both sides" % ell)
    rands = [_rand_fr(nf) for _ in range(count)] if rands is None else rands
    if any(len(r) != nf * FR for r in rands):
        raise ValueError("%d random factors per proof" % nf)
    rec = whisk_shuffle_proof_size(ctx)
    # a wrong length is a fixed-size array mismatch in the reference: reported per item, the library sees a well-formed dummy
    short = [len(p) != rec for p in proofs]
    pf = b"".join(bytes(rec) if s else p for s, p in zip(short, proofs))
    verdict = (ctypes.c_int * count)(*([CPX_ERR_INTERNAL] * count))   # an entry the library does not write is never read as accepted
    pre, post = _in(b"".join(_cat(t) for t in pre_lists)), _in(b"".join(_cat(t) for t in post_lists))
    rechecked = ctypes.c_size_t(0)
    if nf == 8:
        ctx._check(ctx._L.cpx_whisk_verify_shuffle_proofs(ctx._h, count, pre, post, _in(pf), _in(b"".join(rands)), verdict))
    else:
        ctx._check(ctx._L.cpx_whisk_verify_shuffle_proofs_grouped(ctx._h, count, pre, post, _in(pf), _in(b"".join(rands)), verdict, ctypes.byref(rechecked)))
    res = []
    for i, v in enumerate(verdict):
        if short[i]:
            res.append(SerializationError("wrong proof length"))
        elif v == CPX_OK:
            res.append(True)
        elif v == CPX_ERR_VERIFY:
            res.append(False)
        elif v == CPX_ERR_DESERIALIZE:
            res.append(SerializationError("shuffle proof %d" % i))
        else:
            raise CpxError(v, "shuffle proof %d" % i)
    return res, rechecked.value


# ---- a run of shuffles against the resident candidate list (cpx_whisk_candidates_* / cpx_whisk_verify_shuffle_run) ----
def load_candidate_trackers(ctx, trackers):
    """Makes `trackers` (WhiskTracker list, or their bytes back to back) THE candidate list of ctx, decoded once on the device; an empty list
    drops it.  Returns one decoder status per candidate (0 = both points decode and lie in the subgroup; cpx_g1_decompress_status codes).
    An undecodable candidate is not an error here: every item of a run that reads it is a SerializationError, as in the reference."""
    raw = bytes(trackers) if isinstance(trackers, (bytes, bytearray)) else _cat(trackers)
    if len(raw) % (2 * G1POINT_SIZE):
        raise ValueError("a tracker is two 48-byte compressed G1 points")
    n = len(raw) // (2 * G1POINT_SIZE)
    status = _out(n)
    ctx._check(ctx._L.cpx_whisk_candidates_load(ctx._h, n, _in(raw) if n else None, status))
    return list(status[:n])


def candidate_trackers(ctx, first=0, count=None):
    """Candidates first .. first+count-1 of the resident list (count = None: to its end), byte for byte as loaded or as the post trackers
    of an applied item spelt them."""
    if first < 0 or (count is not None and count < 0):
        raise ValueError("first and count are not negative")
    size = ctx._L.cpx_whisk_candidates_size(ctx._h)
    count = max(size - first, 0) if count is None else count
    out = _out(count * 2 * G1POINT_SIZE)
    ctx._check(ctx._L.cpx_whisk_candidates_read(ctx._h, first, count, out))
    ob = bytes(out)
    return [WhiskTracker(ob[96 * i:96 * i + 48], ob[96 * i + 48:96 * i + 96]) for i in range(count)]


def verify_whisk_shuffle_run(ctx, indices_lists, post_lists, proofs, rands=None, grouped=False, apply=True):
    """whisk.rs:106-130 for a run of shuffles over the candidate list of ctx (load_candidate_trackers) in ONE library call.  Item b reads
    the candidates at indices_lists[b] (ell indices) of the list as it stands after items 0..b-1 were written back, whatever their
    results, and post_lists[b] are the trackers it puts there.  rands: per item the verifier's eight factors, twelve when grouped
    (CSPRNG when omitted).  Returns (results, n_applied), or (results, n_applied, n_rechecked) when grouped: results as
    are_valid_whisk_shuffle_proofs (True / False / a SerializationError instance, a wrong proof length among them); the n_applied leading
    accepted items, and no others, have been written back to the resident list.  apply=False is a dry run: the list stays as it was and
    n_applied is None."""
    count = len(indices_lists)
    nf = 12 if grouped else 8
    if len(post_lists) != count or len(proofs) != count or (rands is not None and len(rands) != count):
        raise ValueError("one post tracker list, one proof and one set of factors per index list")
    if count == 0:
        return ([], None if not apply else 0, 0) if grouped else ([], None if not apply else 0)
    ell = ctx.ell
    if any(len(ix) != ell for ix in indices_lists) or any(len(t) != ell for t in post_lists):
        raise ValueError("need exactly ell = %d indices and ell post trackers per item" % ell)
    if any(not 0 <= i < 1 << 32 for ix in indices_lists for i in ix):
        raise ValueError("candidate indices are unsigned 32-bit numbers")
    rands = [_rand_fr(nf) for _ in range(count)] if rands is None else rands
    if any(len(r) != nf * FR for r in rands):
        raise ValueError("%d random factors per proof" % nf)
    rec = whisk_shuffle_proof_size(ctx)
    # a wrong length is a fixed-size array mismatch in the reference: reported per item; the library sees zero bytes, whose M does not decode
    short = [len(p) != rec for p in proofs]
    pf = b"".join(bytes(rec) if s else p for s, p in zip(short, proofs))
    verdict = (ctypes.c_int * count)(*([CPX_ERR_INTERNAL] * count))   # an entry the library does not write is never read as accepted
    idx = (ctypes.c_uint32 * (count * ell))(*[i for ix in indices_lists for i in ix])
    post = _in(b"".join(_cat(t) for t in post_lists))
    applied, rechecked = ctypes.c_size_t(0), ctypes.c_size_t(0)
    p_applied = ctypes.byref(applied) if apply else None
    if grouped:
        ctx._check(ctx._L.cpx_whisk_verify_shuffle_run_grouped(ctx._h, count, idx, post, _in(pf), _in(b"".join(rands)), verdict, p_applied, ctypes.byref(rechecked)))
    else:
        ctx._check(ctx._L.cpx_whisk_verify_shuffle_run(ctx._h, count, idx, post, _in(pf), _in(b"".join(rands)), verdict, p_applied))
    res = []
    for i, v in enumerate(verdict):
        if short[i]:
            res.append(SerializationError("wrong proof length"))
        elif v == CPX_OK:
            res.append(True)
        elif v == CPX_ERR_VERIFY:
            res.append(False)
        elif v == CPX_ERR_DESERIALIZE:
            res.append(SerializationError("shuffle proof %d" % i))
        else:
            raise CpxError(v, "shuffle proof %d" % i)
    n_applied = applied.value if apply else None
    return (res, n_applied, rechecked.value) if grouped else (res, n_applied)


# ---- many tracker proofs per call (cpx_whisk_generate_tracker_proofs / cpx_whisk_verify_tracker_proofs) ----
def generate_whisk_tracker_proofs(ctx, trackers, ks, blinders=None):
    """whisk.rs:228-263 for every (tracker, k, blinder) triple in ONE library call (a constant number of kernel launches).
    ks / blinders: lists of 32-byte wire scalars; omitted blinders come from the OS CSPRNG.  Returns a list of 128-byte proofs, with
    None where the tracker does not decode (the reference's SerializationError); nothing is raised per item."""
    count = len(trackers)
    blinders = [_rand_fr(1) for _ in range(count)] if blinders is None else blinders
    if len(ks) != count or len(blinders) != count:
        raise ValueError("one k and one blinder per tracker")
    if any(len(x) != FR for x in ks) or any(len(x) != FR for x in blinders):
        raise ValueError("k and blinder are 32-byte wire scalars")
    if count == 0:
        return []
    out = _out(TRACKER_PROOF_SIZE * count)
    status = (ctypes.c_int * count)(*([CPX_ERR_INTERNAL] * count))   # an entry the library does not write is never read as a proof
    ctx._check(ctx._L.cpx_whisk_generate_tracker_proofs(ctx._h, count, _in(_cat(trackers)), _in(b"".join(ks)), _in(b"".join(blinders)), out, status))
    blob = bytes(out)
    res = []
    for i, st in enumerate(status):
        if st not in (CPX_OK, CPX_ERR_DESERIALIZE):
            raise CpxError(st, "tracker proof %d" % i)
        res.append(blob[TRACKER_PROOF_SIZE * i:TRACKER_PROOF_SIZE * (i + 1)] if st == CPX_OK else None)
    return res


def are_valid_whisk_tracker_proofs(ctx, trackers, k_commitments, proofs):
    """whisk.rs:183-226 for every (tracker, k_commitment, proof) triple in ONE library call.  Returns a list with True / False, or a
    SerializationError INSTANCE where the reference returns Err (undecodable point, s >= r, wrong length); nothing is raised per item."""
    count = len(trackers)
    if len(k_commitments) != count or len(proofs) != count:
        raise ValueError("one k_commitment and one proof per tracker")
    if count == 0:
        return []
    # a wrong length is a fixed-size array mismatch in the reference: reported per item, the library sees a well-formed dummy
    short = [len(c) != G1POINT_SIZE or len(p) != TRACKER_PROOF_SIZE for c, p in zip(k_commitments, proofs)]
    kc = b"".join(bytes(G1POINT_SIZE) if s else c for s, c in zip(short, k_commitments))
    pf = b"".join(bytes(TRACKER_PROOF_SIZE) if s else p for s, p in zip(short, proofs))
    verdict = (ctypes.c_int * count)(*([CPX_ERR_INTERNAL] * count))   # an entry the library does not write is never read as accepted
    ctx._check(ctx._L.cpx_whisk_verify_tracker_proofs(ctx._h, count, _in(_cat(trackers)), _in(kc), _in(pf), verdict))
    res = []
    for i, v in enumerate(verdict):
        if short[i]:
            res.append(SerializationError("wrong length"))
        elif v == CPX_OK:
            res.append(True)
        elif v == CPX_ERR_VERIFY:
            res.append(False)
        elif v == CPX_ERR_DESERIALIZE:
            res.append(SerializationError("tracker proof %d" % i))
        else:
            raise CpxError(v, "tracker proof %d" % i)
    return res


# ---- the same as ONE multi-scalar multiplication (cpx_whisk_verify_tracker_proofs_grouped / _fused) ----
def _tracker_check_inputs(trackers, k_commitments, proofs, rands):
    """Length checks and marshalling shared by the grouped and the fused call: (count, short, trackers, kc, proofs, rands) as bytes.  An
    item of wrong length is reported per item; the library is handed a dummy that does not decode (zero bytes lack the compression
    flag), so it contributes nothing to any sum and counts as invalid."""
    count = len(trackers)
    if len(k_commitments) != count or len(proofs) != count or (rands is not None and len(rands) != count):
        raise ValueError("one k_commitment, one proof and one pair of weights per tracker")
    rands = [_rand_fr(2) for _ in range(count)] if rands is None else rands
    if any(len(r) != 2 * FR for r in rands):
        raise ValueError("two 32-byte weights per item")
    short = [len(c) != G1POINT_SIZE or len(p) != TRACKER_PROOF_SIZE for c, p in zip(k_commitments, proofs)]
    kc = b"".join(bytes(G1POINT_SIZE) if s else c for s, c in zip(short, k_commitments))
    pf = b"".join(bytes(TRACKER_PROOF_SIZE) if s else p for s, p in zip(short, proofs))
    return count, short, _cat(trackers), kc, pf, b"".join(rands)


def are_valid_whisk_tracker_proofs_grouped(ctx, trackers, k_commitments, proofs, rands=None):
    """are_valid_whisk_tracker_proofs through the grouped check (cpx_whisk_verify_tracker_proofs_grouped): every group of items is one MSM of
    five points per item, and only the items of a group whose sum is not the identity get the per-item relations.  rands: one 64-byte
    pair of weights (a_i || b_i, wire scalars, non-zero) per item, from the OS CSPRNG when omitted.  Returns (results as
    are_valid_whisk_tracker_proofs, n_rechecked); context option "locate_groups_max" sets the grouping."""
    count, short, tr, kc, pf, rnd = _tracker_check_inputs(trackers, k_commitments, proofs, rands)
    if count == 0:
        return [], 0
    verdict = (ctypes.c_int * count)(*([CPX_ERR_INTERNAL] * count))   # an entry the library does not write is never read as accepted
    rechecked = ctypes.c_size_t(0)
    ctx._check(ctx._L.cpx_whisk_verify_tracker_proofs_grouped(ctx._h, count, _in(tr), _in(kc), _in(pf), _in(rnd), verdict, ctypes.byref(rechecked)))
    res = []
    for i, v in enumerate(verdict):
        if short[i]:
            res.append(SerializationError("wrong length"))
        elif v == CPX_OK:
            res.append(True)
        elif v == CPX_ERR_VERIFY:
            res.append(False)
        elif v == CPX_ERR_DESERIALIZE:
            res.append(SerializationError("tracker proof %d" % i))
        else:
            raise CpxError(v, "tracker proof %d" % i)
    return res, rechecked.value


def whisk_tracker_proofs_partial(ctx, trackers, k_commitments, proofs, rands=None):
    """cpx_whisk_verify_tracker_proofs_fused: (partial_jac, n_invalid) — the 144-byte Jacobian sum of the weighted relations of all items that
    decode, and the number of items that do not (wrong lengths included).  The batch is accepted iff n_invalid == 0 and the partials of
    all calls, contexts and GPUs — the shuffle proofs' among them — add up to the identity (Context.sum_jac)."""
    count, short, tr, kc, pf, rnd = _tracker_check_inputs(trackers, k_commitments, proofs, rands)
    from . import JAC
    partial = _out(JAC)
    n_invalid = ctypes.c_int(0)
    ctx._check(ctx._L.cpx_whisk_verify_tracker_proofs_fused(ctx._h, count, _in(tr), _in(kc), _in(pf), _in(rnd), partial, ctypes.byref(n_invalid)))
    return bytes(partial), n_invalid.value


def are_all_valid_whisk_tracker_proofs(ctx, trackers, k_commitments, proofs, rands=None):
    """All-or-nothing: True iff every item decodes and the weighted sum of all relations is the identity"""
    partial, n_invalid = whisk_tracker_proofs_partial(ctx, trackers, k_commitments, proofs, rands)
    return n_invalid == 0 and bool(ctx.sum_jac(partial)[1])


# ---- many trackers and k commitments per call (cpx_whisk_trackers_from_k_r / cpx_g1_generator_mul) ----
def trackers_from_k_r(ctx, ks, rs):
    """whisk.rs:45-55 WhiskTracker::from_k_r and whisk.rs:370 get_k_commitment for every (k, r) pair in ONE library call, on the fixed-base
    table of the generator.  ks / rs: lists of 32-byte wire scalars.  Returns (list of WhiskTracker, list of 48-byte k commitments)."""
    count = len(ks)
    if len(rs) != count:
        raise ValueError("one r per k")
    if any(len(x) != FR for x in ks) or any(len(x) != FR for x in rs):
        raise ValueError("k and r are 32-byte wire scalars")
    if count == 0:
        return [], []
    trk, kc = _out(2 * G1POINT_SIZE * count), _out(G1POINT_SIZE * count)
    ctx._check(ctx._L.cpx_whisk_trackers_from_k_r(ctx._h, count, _in(b"".join(ks)), _in(b"".join(rs)), trk, kc))
    tb, cb = bytes(trk), bytes(kc)
    return ([WhiskTracker(tb[96 * i:96 * i + 48], tb[96 * i + 48:96 * i + 96]) for i in range(count)],
            [cb[48 * i:48 * (i + 1)] for i in range(count)])


def k_commitments(ctx, ks):
    """whisk.rs:370 get_k_commitment for every k in ONE library call: the 48-byte encodings of k_i * G"""
    if any(len(x) != FR for x in ks):
        raise ValueError("k is a 32-byte wire scalar")
    if not ks:
        return []
    cb = ctx.generator_mul(b"".join(ks), compressed=True)[1]
    return [cb[48 * i:48 * (i + 1)] for i in range(len(ks))]


# ---- which trackers a set of keys opens (cpx_whisk_find_trackers) ----
def find_trackers(ctx, trackers, ks):
    """The relation of whisk.rs:36-55, k * r_G == k_r_G, for every (tracker, key) pair in ONE library call.  ks: list of 32-byte wire scalars.
    Returns (owners, status): owners[i] is the smallest index j whose key opens tracker i (an int) or None; status[i] is True, or a
    SerializationError INSTANCE where a half of the tracker does not decode (its owner is None); nothing is raised per item.  A tracker
    whose two halves are the identity is opened by every key (owner 0); of duplicate keys the smaller index is reported."""
    if any(len(x) != FR for x in ks):
        raise ValueError("k is a 32-byte wire scalar")
    n, nk = len(trackers), len(ks)
    if n > 1 << 23 or nk > 1 << 20 or n * nk > 1 << 32:
        raise ValueError("at most 2^23 trackers, 2^20 keys and 2^32 pairs per call")
    if n == 0:
        return [], []
    owner = (ctypes.c_uint32 * n)(*([CPX_NO_OWNER] * n))
    status = (ctypes.c_int * n)(*([CPX_ERR_INTERNAL] * n))   # an entry the library does not write is never read as an owner
    ctx._check(ctx._L.cpx_whisk_find_trackers(ctx._h, n, _in(_cat(trackers)), nk, _in(b"".join(ks)) if nk else None, owner, status))
    owners, res = [], []
    for i, st in enumerate(status):
        if st not in (CPX_OK, CPX_ERR_DESERIALIZE):
            raise CpxError(st, "tracker %d" % i)
        res.append(True if st == CPX_OK else SerializationError("tracker %d" % i))
        owners.append(int(owner[i]) if st == CPX_OK and owner[i] != CPX_NO_OWNER else None)
    return owners, res


# ---- small helpers of whisk.rs:295-345 ----
def to_bytes_g1affine(ctx, g1):
    """whisk.rs:307-311: affine wire point (96 B) -> 48-byte compressed encoding"""
    from . import JAC
    one = pr.fp_to_wire(1)
    jac = g1 + (bytes(48) if g1 == bytes(AFF) else one)
    assert len(jac) == JAC
    return ctx.normalize(jac, compressed=True)[1]


def from_bytes_g1affine(ctx, buf):
    """whisk.rs:313-315: validated decompression (on curve, in the subgroup)"""
    try:
        return ctx.decompress(buf, check_subgroup=True)
    except CpxError as e:
        if e.code == CPX_ERR_DESERIALIZE:
            raise SerializationError(str(e))
        raise


def g1_generator(ctx):
    """whisk.rs:318-320"""
    return pr.g1_generator_wire()


def bls_g1_scalar_multiply(ctx, g1, scalar):
    """whisk.rs:323-325"""
    return ctx.scale(g1, scalar)


def rand_scalar():
    """whisk.rs:328-330 (CSPRNG instead of a caller-supplied rng)"""
    return _rand_fr(1)


def to_bytes_fr(fr):
    """whisk.rs:333-337: wire scalar -> 32-byte little-endian canonical"""
    return pr.fr_from_wire(fr).to_bytes(32, "little")


def from_bytes_fr(b):
    """whisk.rs:343-345: little-endian bytes, reduced mod r"""
    return pr.fr_to_wire(int.from_bytes(b, "little"))
