"""CPU checks of the batched tracker-proof entry points (cpx_whisk_generate_tracker_proofs / cpx_whisk_verify_tracker_proofs): the
boundary — header, export list, library, Rust declarations, argument checks that need no device — and the schedule of the verifier's
two-base joint ladder (curdleproofs_amd/csrc/tracker_ladder.hpp), run on the CPU by tests/host_emul/tracker_ladder_emul.cpp with the
one-lane host build of the g1_28.hpp additions and compared with the oracle's scalar multiplications and addition."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("cpx_whisk_generate_tracker_proofs", "cpx_whisk_verify_tracker_proofs")
R_ = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
Z2 = 0xd201000000010000 ** 2          # the endomorphism's eigenvalue is -z^2: where the split k = t + q z^2 changes its upper half
FR, AFF, JAC = 32, 96, 144


@pytest.fixture(scope="module")
def lib():
    from curdleproofs_amd.build import build
    build()
    import curdleproofs_amd as cpx
    return cpx.load_library()


def test_header_declares_both_calls_beside_their_reference_lines():
    hdr = open(os.path.join(ROOT, "include", "cpx.h")).read()
    for name, cite in zip(NAMES, ("whisk.rs:228-263", "whisk.rs:183-226")):
        at = hdr.index("int %s(" % name)
        comment = hdr[hdr.rindex("/*", 0, at):at]      # the comment block that ends right above the declaration
        assert cite in comment, "%s: %s is not cited beside the declaration" % (name, cite)
        assert comment.rstrip().endswith("*/")


def test_names_are_exported_everywhere(lib):
    import curdleproofs_amd as cpx
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in NAMES:
        assert name in cpx.EXPORTS
        assert hasattr(lib, name), "libcpx.so does not export %s" % name
        assert re.search(r"pub fn %s\(" % name, ffi), "integration/rust/ffi.rs lacks %s" % name
    assert "k_tracker_challenge" in cpx.Context.KERNELS and "k_tracker_relations" in cpx.Context.KERNELS


def test_null_arguments_are_rejected_without_a_device(lib):
    import curdleproofs_amd as cpx
    buf = (ctypes.c_uint8 * 128)()
    st = (ctypes.c_int * 1)(7)
    # NULL data pointers with count > 0 (checked before the context is looked at), and a NULL context
    assert lib.cpx_whisk_generate_tracker_proofs(None, 1, None, None, None, None, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_verify_tracker_proofs(None, 1, None, None, None, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_generate_tracker_proofs(None, 1, buf, buf, buf, buf, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_verify_tracker_proofs(None, 1, buf, buf, None, st) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_verify_tracker_proofs(None, 1, buf, buf, buf, st) == cpx.CPX_ERR_ARG
    assert st[0] == 7


def test_python_wrappers_check_lengths_before_touching_the_library():
    from curdleproofs_amd import whisk
    t = whisk.WhiskTracker(b"\x01" * 48, b"\x02" * 48)
    ctx = None                                             # any use of the context would raise AttributeError, not ValueError
    with pytest.raises(ValueError):
        whisk.are_valid_whisk_tracker_proofs(ctx, [t, t], [bytes(48)], [bytes(128), bytes(128)])
    with pytest.raises(ValueError):
        whisk.are_valid_whisk_tracker_proofs(ctx, [t], [bytes(48)], [])
    with pytest.raises(ValueError):
        whisk.generate_whisk_tracker_proofs(ctx, [t, t], [bytes(32)], [bytes(32), bytes(32)])
    with pytest.raises(ValueError):
        whisk.generate_whisk_tracker_proofs(ctx, [t], [bytes(32)], [bytes(32), bytes(32)])
    with pytest.raises(ValueError):
        whisk.generate_whisk_tracker_proofs(ctx, [t], [bytes(31)], [bytes(32)])
    assert whisk.are_valid_whisk_tracker_proofs(ctx, [], [], []) == [] and whisk.generate_whisk_tracker_proofs(ctx, [], [], []) == []


# ---- the ladder schedule on the CPU ----
@pytest.fixture(scope="module")
def emul():
    src = os.path.join(HERE, "host_emul", "tracker_ladder_emul.cpp")
    so = os.path.join(HERE, "host_emul", "_tracker_ladder.so")
    csrc = os.path.join(ROOT, "curdleproofs_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("tracker_ladder.hpp", "recode.hpp", "glv.hpp", "g1_28.hpp", "fp28.hpp", "g1.hpp", "mont32.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.emul_tracker_ladder.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, vp]
    L.emul_tracker_ladder.restype = None
    return L


def _scalars(orc):
    """{0, 1, 2, r - 1, r - 2, the two scalars at the boundary of the endomorphism split, 8 seeded random}, as integers"""
    rnd = orc.fr_to_canonical_bytes(orc.rng(4242).fr(8))
    return [0, 1, 2, R_ - 1, R_ - 2, Z2, Z2 - 1] + [int.from_bytes(rnd[FR * i:FR * (i + 1)], "little") for i in range(8)]


def _neg(orc, p):
    return orc.g1_scale(p, orc.fr_from_canonical_bytes((R_ - 1).to_bytes(32, "little")))


def test_joint_ladder_schedule_matches_the_oracle(emul, orc):
    from curdleproofs_amd import params
    rng = orc.rng(99)
    P, Q = rng.g1_affine(1), rng.g1_affine(1)
    ident = bytes(AFF)
    pairs = {"random_random": (P, Q), "same_point": (P, P), "opposite_points": (P, _neg(orc, P)), "second_is_identity": (P, ident)}
    scal = _scalars(orc)
    assert len(scal) == 15
    cases = [(a, b) for a in scal for b in scal]
    n = len(cases)
    sa = b"".join(a.to_bytes(32, "little") for a, _ in cases)
    sb = b"".join(b.to_bytes(32, "little") for _, b in cases)
    wa, wb = orc.fr_from_canonical_bytes(sa), orc.fr_from_canonical_bytes(sb)
    one = params.fp_to_wire(1)
    jac = lambda aff: aff + (bytes(48) if aff == ident else one)
    for name, (p1, p2) in pairs.items():
        out = ctypes.create_string_buffer(JAC * n)
        adds = (ctypes.c_int * n)()
        emul.emul_tracker_ladder(n, p1 * n, p2 * n, sa, sb, out, adds)
        got = orc.g1_compress_jac(out.raw)
        t1, t2 = orc.g1_scale(p1 * n, wa), orc.g1_scale(p2 * n, wb)
        for i, (a, b) in enumerate(cases):
            want = orc.g1_compress_jac(orc.g1_add_jac(jac(t1[AFF * i:AFF * (i + 1)]), jac(t2[AFF * i:AFF * (i + 1)])))
            assert got[48 * i:48 * (i + 1)] == want, "%s: %#x * P1 + %#x * P2" % (name, a, b)
        # at most one addition per base and step; none at all for two zero scalars
        assert max(adds) <= 2 * 129 and adds[0] == 0
    # the pairs above do meet the exceptional branch: 1 * P + 1 * P doubles, 1 * P + 1 * (-P) cancels
    i11 = cases.index((1, 1))
    out = ctypes.create_string_buffer(JAC * n)
    emul.emul_tracker_ladder(n, P * n, P * n, sa, sb, out, None)
    assert orc.g1_compress_jac(out.raw[JAC * i11:JAC * (i11 + 1)]) == orc.g1_compress(orc.g1_scale(P, orc.fr_from_u64(2)))
    emul.emul_tracker_ladder(n, P * n, _neg(orc, P) * n, sa, sb, out, None)
    assert orc.g1_compress_jac(out.raw[JAC * i11:JAC * (i11 + 1)]) == bytes([0xc0]) + bytes(47)
