"""Reference decoder for compressed G1 encodings and the corpus of encodings the decoding tests run.

A big-integer restatement of ark's `G1Affine::deserialize_compressed` (Compress::Yes, Validate::Yes) as oracle/g1.h
`g1_decompress` states it: 48 bytes big-endian x, byte 0 bit 7 = compressed, bit 6 = infinity, bit 5 = sort (y > p - y).
p = 3 mod 4, so the square root candidate is rhs^((p+1)/4).  Membership in the order-r subgroup is asked of the oracle
(`orc.g1_in_subgroup`): this module restates the parsing, the range test, the square root and the sign choice.

`decode` returns (status, x, y): status 0 = ok, 1 = malformed or off the curve, 2 = on the curve but outside the subgroup
(the status bytes of cpx_g1_decompress_status); (x, y) = None for the identity and for every rejected encoding.
The corpus is deterministic; tests/test_decoding_reference_cpu.py pins this module to the oracle on all of it, and
tests/test_gpu_decoding.py compares every GPU decoding path with it."""
import hashlib

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
B_COEFF = 4
AFF = 96

OK, MALFORMED, NOT_IN_SUBGROUP = 0, 1, 2
FLAG_BYTES = (0x00, 0x20, 0x40, 0x60, 0x80, 0xa0, 0xc0, 0xe0)   # every combination of compressed / infinity / sort


def is_qr(a):
    return a % P == 0 or pow(a, (P - 1) // 2, P) == 1


def rhs(x):
    return (x * x * x + B_COEFF) % P


def fp_wire(v):
    """canonical integer -> the 48-byte Montgomery limbs of the wire form (include/cpx.h)"""
    return (v * (1 << 384) % P).to_bytes(48, "little")


def aff_wire(pt):
    """(x, y) or None (identity) -> 96-byte affine wire record"""
    return bytes(AFF) if pt is None else fp_wire(pt[0]) + fp_wire(pt[1])


def aff_from_wire(b):
    if b == bytes(AFF):
        return None
    inv = pow(1 << 384, -1, P)
    return (int.from_bytes(b[:48], "little") * inv % P, int.from_bytes(b[48:96], "little") * inv % P)


def encode(x, flags):
    """flag bits OR-ed into byte 0 of the 48-byte big-endian x (x may be >= p: the decoder must refuse those)"""
    assert 0 <= x < 1 << 381
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


def compress(pt):
    """(x, y) or None -> canonical compressed encoding"""
    if pt is None:
        return bytes([0xc0]) + bytes(47)
    x, y = pt
    return encode(x, 0x80 | (0x20 if y > P - y else 0))


def decode(enc, orc, strict_infinity=False, check_subgroup=True):
    assert len(enc) == 48
    b0 = enc[0]
    compressed, infinity, sort = bool(b0 & 0x80), bool(b0 & 0x40), bool(b0 & 0x20)
    x = int.from_bytes(bytes([b0 & 0x1f]) + enc[1:], "big")
    if not compressed:
        return MALFORMED, None, None
    if infinity:
        # ark-bls12-381 ^0.4 returns the identity as soon as both flags are set; strict = only 0xc0 || 0^47
        if strict_infinity and (sort or x != 0):
            return MALFORMED, None, None
        return OK, None, None
    if x >= P:
        return MALFORMED, None, None
    r = rhs(x)
    y = pow(r, (P + 1) // 4, P)
    if y * y % P != r:
        return MALFORMED, None, None
    small, large = min(y, P - y), max(y, P - y)   # (y = 0 would need x^3 = -4: no such x in Fp, see test_no_two_torsion)
    y = large if sort else small
    if check_subgroup and not orc.g1_in_subgroup(aff_wire((x, y))):
        return NOT_IN_SUBGROUP, None, None
    return OK, x, y


def expected_output(enc, orc, strict_infinity, check_subgroup):
    """(status byte, 96-byte affine record) that cpx_g1_decompress_status must produce for `enc`: the identity in place of
    every rejected point"""
    st, x, y = decode(enc, orc, strict_infinity, check_subgroup)
    return st, aff_wire(None if st or x is None else (x, y))


def _hash_x(tag, i):
    h = hashlib.sha512(tag + i.to_bytes(8, "big")).digest()
    return int.from_bytes(h, "big") % P


def off_curve_xs(count):
    """x < p whose x^3 + 4 is a non-residue (no point of E has that x)"""
    out, i = [], 0
    while len(out) < count:
        x = _hash_x(b"off curve", i)
        i += 1
        if not is_qr(rhs(x)):
            out.append(x)
    return out


def non_member_points(orc, count):
    """points of E(Fp) outside the order-r subgroup (E(Fp) has order h * r with h ~ 2^126: a point found from a random x is
    outside the subgroup with overwhelming probability; the oracle confirms each)"""
    out, i = [], 0
    while len(out) < count:
        x = _hash_x(b"outside the subgroup", i)
        i += 1
        r = rhs(x)
        if not is_qr(r):
            continue
        y = pow(r, (P + 1) // 4, P)
        y = min(y, P - y)
        assert orc.g1_on_curve(aff_wire((x, y)))
        if not orc.g1_in_subgroup(aff_wire((x, y))):
            out.append((x, y))
    return out


def subgroup_points(orc, count, seed=2718):
    b = orc.rng(seed).g1_affine(count)
    return [aff_from_wire(b[AFF * i:AFF * (i + 1)]) for i in range(count)]


def corpus(orc):
    """[(label, 48-byte encoding)]: accepted and refused encodings at every edge of the decoder"""
    cases = []
    valid = subgroup_points(orc, 6)
    for i, pt in enumerate(valid):
        enc = compress(pt)
        cases.append(("subgroup[%d]" % i, enc))
        cases.append(("subgroup[%d] sort flipped (-P)" % i, bytes([enc[0] ^ 0x20]) + enc[1:]))
    off = off_curve_xs(4)
    for i, x in enumerate(off):
        cases.append(("off curve[%d]" % i, encode(x, 0x80)))
        cases.append(("off curve[%d] sort" % i, encode(x, 0xa0)))
    nm = non_member_points(orc, 4)
    for i, (x, y) in enumerate(nm):
        cases.append(("non-member[%d]" % i, encode(x, 0x80)))
        cases.append(("non-member[%d] sort" % i, encode(x, 0xa0)))
    # the named x values under every flag byte; 0xc0 / 0xe0 with x bits set are the non-canonical infinities
    special = [("x=0", 0), ("x=1", 1), ("x=p-1", P - 1), ("x=p", P), ("x=p+1", P + 1), ("x=2^381-1", (1 << 381) - 1),
               ("x=off curve", off[0]), ("x=non-member", nm[0][0]), ("x=subgroup", valid[0][0])]
    for name, x in special:
        for f in FLAG_BYTES:
            cases.append(("%s flags %02x" % (name, f), encode(x, f)))
    cases.append(("0xc0 last byte 1", bytes([0xc0]) + bytes(46) + b"\x01"))
    cases.append(("0xc0 second byte 1", bytes([0xc0, 0x01]) + bytes(46)))
    seen, out = set(), []
    for label, enc in cases:   # (the flag sweep repeats a few encodings of the lists above: keep the first label)
        if enc not in seen:
            seen.add(enc)
            out.append((label, enc))
    return out


# ---- proof layout (CurdleproofsProof::serialize, curdleproofs.rs:300-310 and the sub-proofs' serialisers) ----

SCALAR_SLOTS = ("r_p", "c", "d", "z_k", "z_t", "z_u", "x")
L_VECTORS = ("L_C", "R_C", "L_D", "R_D", "L_A", "L_T", "L_U", "R_A", "R_T", "R_U")


def proof_layout(ell):
    """(points, scalars): [(name, byte offset)] of the 18 + 10 L proof points in slot order and {name: offset} of the seven
    scalars, from the serialisation order itself"""
    L = (ell + 4).bit_length() - 1
    points, scalars, o = [], {}, 0

    def pts(*names):
        nonlocal o
        for nm in names:
            points.append((nm, o))
            o += 48

    def vec(name):
        pts(*("%s[%d]" % (name, j) for j in range(L)))

    def sc(*names):
        nonlocal o
        for nm in names:
            scalars[nm] = o
            o += 32

    pts("A", "cm_T.T1", "cm_T.T2", "cm_U.T1", "cm_U.T2", "R", "S", "B", "C")   # curdleproofs.rs:300-310, SamePerm B, GrandProduct C
    sc("r_p")
    pts("B_c", "B_d")                                                           # IPA
    for v in ("L_C", "R_C", "L_D", "R_D"):
        vec(v)
    sc("c", "d")
    pts("cm_A.T1", "cm_A.T2", "cm_B.T1", "cm_B.T2")                             # SameScalar
    sc("z_k", "z_t", "z_u")
    pts("B_a", "B_t", "B_u")                                                    # SameMultiscalar
    for v in ("L_A", "L_T", "L_U", "R_A", "R_T", "R_U"):
        vec(v)
    sc("x")
    assert len(points) == 18 + 10 * L and o == 48 * len(points) + 32 * 7
    return points, scalars


def noncanonical_scalars():
    return {"r": R, "r+1": R + 1, "r+2^128": R + (1 << 128), "2^256-1": (1 << 256) - 1}


def canonical_edge_scalars():
    """r - 1 and the largest value below r whose top 32-bit word is one less than r's (every lower word all ones)"""
    top = R >> 224
    return {"r-1": R - 1, "top word of r - 1, rest ones": (top - 1) * (1 << 224) + (1 << 224) - 1}


def point_defects(orc, original):
    """the five point defects, cycled over the proof slots: [(name, encoding)] given the slot's original encoding"""
    x_off = off_curve_xs(1)[0]
    nm = non_member_points(orc, 1)[0]
    return [("off curve", encode(x_off, 0x80)),
            ("x = p", encode(P, 0x80)),
            ("x = 0 (3-torsion)", encode(0, 0x80)),
            ("non-member", encode(nm[0], 0x80)),
            ("no compression flag", bytes([original[0] & 0x7f]) + original[1:])]
