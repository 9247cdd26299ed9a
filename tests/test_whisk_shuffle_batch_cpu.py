"""CPU checks of the batched shuffle entry points (cpx_batch_shuffle, cpx_whisk_generate_shuffle_proofs, cpx_whisk_verify_shuffle_proofs):
the boundary — header, export list, library, Rust declarations, argument checks that need no device, the Python mirrors' shape errors —
and the index arithmetic host and kernels share (curdleproofs_amd/csrc/shuffle_plan.hpp), run on the CPU by
tests/host_emul/shuffle_plan_emul.cpp and compared with plain Python."""
import ctypes
import os
import random
import re
import subprocess
import types

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("cpx_batch_shuffle", "cpx_whisk_generate_shuffle_proofs", "cpx_whisk_verify_shuffle_proofs")
KERNELS = ("k_shuffle_status", "k_shuffle_gather", "k_shuffle_commit")
ELLS = (4, 28, 124)
COUNTS = (1, 3, 65)


@pytest.fixture(scope="module")
def lib():
    from curdleproofs_amd.build import build
    build()
    import curdleproofs_amd as cpx
    return cpx.load_library()


def test_header_declares_the_calls_beside_their_reference_lines():
    hdr = open(os.path.join(ROOT, "include", "cpx.h")).read()
    for name, cite in zip(NAMES, ("util.rs:83-106", "whisk.rs:144-179", "whisk.rs:106-130")):
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
    for k in KERNELS:
        assert k in cpx.Context.KERNELS
        assert not k.startswith(("k_msm_fix", "k_msm_tblw", "k_msm_accw"))      # the prefixes bench.py prices


def test_null_arguments_and_count_zero_without_a_device(lib):
    import curdleproofs_amd as cpx
    buf = (ctypes.c_uint8 * 8192)(*([0xaa] * 8192))
    st = (ctypes.c_int * 1)(7)
    # NULL data pointers with count > 0 (checked before the context is looked at), and a NULL context
    assert lib.cpx_batch_shuffle(None, 1, None, None, None, None, None, None, None, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_batch_shuffle(None, 1, buf, buf, buf, buf, None, buf, buf, buf) == cpx.CPX_ERR_ARG
    assert lib.cpx_batch_shuffle(None, 1, buf, buf, buf, buf, buf, buf, buf, buf) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_generate_shuffle_proofs(None, 1, None, None, None, None, None, None, None, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_generate_shuffle_proofs(None, 1, buf, buf, buf, buf, buf, buf, buf, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_generate_shuffle_proofs(None, 1, buf, buf, buf, buf, buf, buf, buf, st) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_verify_shuffle_proofs(None, 1, None, None, None, None, None) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_verify_shuffle_proofs(None, 1, buf, buf, None, buf, st) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_verify_shuffle_proofs(None, 1, buf, buf, buf, buf, st) == cpx.CPX_ERR_ARG
    # count = 0 touches no buffer (without a context there is nothing to run on: still CPX_ERR_ARG, and still nothing written)
    assert lib.cpx_whisk_verify_shuffle_proofs(None, 0, None, None, None, None, None) == cpx.CPX_ERR_ARG
    assert st[0] == 7 and bytes(buf) == b"\xaa" * 8192


def test_python_mirrors_check_shapes_before_touching_the_library():
    from curdleproofs_amd import util, whisk
    ell = 4
    ctx = types.SimpleNamespace(ell=ell, n=ell + 4)        # any use of the library would raise AttributeError, not ValueError
    t = whisk.WhiskTracker(b"\x01" * 48, b"\x02" * 48)
    one = [t] * ell
    perm, k, mb, rand = list(range(ell)), bytes(32), bytes(128), bytes(32 * (3 * 8 + 9))
    with pytest.raises(ValueError):                        # one permutation per tracker list
        whisk.generate_whisk_shuffle_proofs(ctx, [one, one], permutations=[perm])
    with pytest.raises(ValueError):                        # ell trackers per list
        whisk.generate_whisk_shuffle_proofs(ctx, [one[:-1]], [perm], [k], [mb], [rand])
    with pytest.raises(ValueError):                        # 32-byte scalars
        whisk.generate_whisk_shuffle_proofs(ctx, [one], [perm], [k[:31]], [mb], [rand])
    with pytest.raises(ValueError):
        whisk.generate_whisk_shuffle_proofs(ctx, [one], [perm], [k], [mb[:96]], [rand])
    with pytest.raises(ValueError):
        whisk.generate_whisk_shuffle_proofs(ctx, [one], [perm + [0]], [k], [mb], [rand])
    with pytest.raises(ValueError):
        whisk.are_valid_whisk_shuffle_proofs(ctx, [one, one], [one], [b"", b""])
    with pytest.raises(ValueError):
        whisk.are_valid_whisk_shuffle_proofs(ctx, [one], [one[:-1]], [b""])
    with pytest.raises(ValueError):
        whisk.are_valid_whisk_shuffle_proofs(ctx, [one], [one], [b""], rands=[bytes(32 * 7)])
    with pytest.raises(ValueError):
        util.shuffle_permute_and_commit_inputs(ctx, [bytes(96 * ell)], [bytes(96 * ell)], [perm, perm], [k], [mb])
    with pytest.raises(ValueError):
        util.shuffle_permute_and_commit_inputs(ctx, [bytes(96 * ell)], [bytes(96 * (ell - 1))], [perm], [k], [mb])
    assert whisk.generate_whisk_shuffle_proofs(None, []) == [] and whisk.are_valid_whisk_shuffle_proofs(None, [], [], []) == []
    assert util.shuffle_permute_and_commit_inputs(ctx, [], [], [], [], []) == []


# ---- the shared index header on the CPU ----
@pytest.fixture(scope="module")
def emul():
    src = os.path.join(HERE, "host_emul", "shuffle_plan_emul.cpp")
    so = os.path.join(HERE, "host_emul", "_shuffle_plan.so")
    csrc = os.path.join(ROOT, "curdleproofs_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("shuffle_plan.hpp", "mont32.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    for f in ("emul_shuffle_sizes", "emul_shuffle_offsets", "emul_shuffle_fold", "emul_shuffle_placeholder", "emul_shuffle_gather"):
        getattr(L, f).restype = None
    return L


def _u64(n):
    return (ctypes.c_uint64 * max(n, 1))()


def _sizes(emul, count, ell, verifier):
    s = _u64(5)
    emul.emul_shuffle_sizes(count, ell, verifier, s)
    return dict(planes=s[0], points=s[1], upload=s[2], plane_points=s[3], fits=s[4])


@pytest.mark.parametrize("verifier", [0, 1], ids=["prover", "verifier"])
@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("count", COUNTS)
def test_every_offset_and_destination_is_in_range_and_hit_once(emul, count, ell, verifier):
    sz = _sizes(emul, count, ell, verifier)
    planes = 4 if verifier else 2
    npts = planes * count * ell + (count if verifier else 0)
    upload = (2 * count * ell * 96 + 48 * count) if verifier else count * ell * 96
    assert sz == dict(planes=planes, points=npts, upload=upload, plane_points=count * ell, fits=1)
    off, idx, midx = _u64(npts), _u64(planes * count * ell), _u64(count)
    emul.emul_shuffle_offsets(count, ell, verifier, off, idx, midx)
    # plain Python: tracker e of item i on side s (0 pre, 1 post) starts at (s * count * ell + i * ell + e) * 96; r_G first, k_r_G 48 bytes on
    want = {}
    for pl in range(planes):
        for i in range(count):
            for e in range(ell):
                want[(pl * count + i) * ell + e] = ((pl >> 1) * count * ell + i * ell + e) * 96 + 48 * (pl & 1)
    assert [idx[j] for j in range(planes * count * ell)] == list(range(planes * count * ell))      # dense plane-major, every slot once
    assert all(off[idx[j]] == want[j] for j in want)
    if verifier:
        assert [midx[i] for i in range(count)] == [4 * count * ell + i for i in range(count)]
        assert [off[midx[i]] for i in range(count)] == [2 * count * ell * 96 + 48 * i for i in range(count)]
    offs = [off[j] for j in range(npts)]
    assert len(set(offs)) == npts and all(o % 48 == 0 and o + 48 <= upload for o in offs)
    assert sorted(offs) == list(range(0, upload, 48))          # every encoding of the upload is decoded exactly once


@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("count", COUNTS)
def test_gather_destinations_and_sources(emul, count, ell):
    rnd = random.Random(1000 * count + ell)
    n = count * ell
    perm = []
    for i in range(count):
        p = list(range(ell))
        rnd.shuffle(p)
        perm += p
    kr, ks = [rnd.getrandbits(32) for _ in range(n)], [rnd.getrandbits(32) for _ in range(n)]
    arr = lambda v: (ctypes.c_uint32 * len(v))(*v)
    for label, pm in (("permutations", perm), ("entries that are no index", [0xffffffff if g % 5 == 0 else ell + g for g in range(n)])):
        t, u, z, src = arr([0] * n), arr([0] * n), arr([0] * 2 * n), _u64(n)
        emul.emul_shuffle_gather(count, ell, arr(pm), arr(kr), arr(ks), t, u, z, src)
        assert all(ell * (g // ell) <= src[g] < ell * (g // ell + 1) for g in range(n)), label      # a row never reads outside itself
        if pm is perm:
            assert [src[g] for g in range(n)] == [ell * (g // ell) + perm[g] for g in range(n)]
            assert sorted(src[g] for g in range(n)) == list(range(n))                                # every element read exactly once
        else:
            assert [src[g] for g in range(n)] == list(range(n))
        assert list(t) == [kr[src[g]] for g in range(n)] and list(u) == [ks[src[g]] for g in range(n)]
        assert list(z) == [v for g in range(n) for v in (kr[src[g]], ks[src[g]])]                    # (T_j, U_j) interleaved: zip_trackers


@pytest.mark.parametrize("verifier", [0, 1], ids=["prover", "verifier"])
@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("count", COUNTS)
def test_status_fold_and_placeholder(emul, count, ell, verifier):
    planes = 4 if verifier else 2
    pp = count * ell
    npts = planes * pp + (count if verifier else 0)
    per_item = lambda i: [pl * pp + i * ell + e for pl in range(planes) for e in range(ell)] + ([4 * pp + i] if verifier else [])
    cases = {"none": []}
    for i in sorted({0, count // 2, count - 1}):
        pts = per_item(i)
        cases["first point of item %d" % i] = [pts[0]]
        cases["last tracker point of item %d" % i] = [pts[planes * ell - 1]]
        cases["a middle point of item %d" % i] = [pts[len(pts) // 2]]
        if verifier:
            cases["M of item %d" % i] = [pts[-1]]
    cases["two items"] = [per_item(0)[1], per_item(count - 1)[-1]]
    for label, bad_points in cases.items():
        status = (ctypes.c_uint8 * npts)()
        for k, j in enumerate(bad_points):
            status[j] = 1 + k % 2                       # both non-zero verdicts of the decoder count
        want = [1 if any(status[j] for j in per_item(i)) else 0 for i in range(count)]
        bad, bad_lanes = (ctypes.c_uint8 * count)(), (ctypes.c_uint8 * count)()
        emul.emul_shuffle_fold(count, ell, verifier, status, 64, bad, bad_lanes)
        assert list(bad) == want and list(bad_lanes) == want, label
        pts = (ctypes.c_uint32 * npts)(*range(1, npts + 1))
        gen = 0xabcdef01
        emul.emul_shuffle_placeholder(count, ell, verifier, status, pts, gen)
        for i in range(count):
            for j in per_item(i):
                assert pts[j] == (gen if want[i] else j + 1), (label, i, j)     # a bad item's rows are the placeholder, the others untouched
