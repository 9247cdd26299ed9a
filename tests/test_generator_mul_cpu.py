"""CPU checks of the generator's fixed-base table (cpx_g1_generator_mul / cpx_whisk_trackers_from_k_r): the boundary — header, export
list, library, Rust declarations, argument checks that need no device — and curdleproofs_amd/csrc/gen_table.hpp, compiled with g++ as
tests/host_emul/gen_table_emul.cpp and compared with Python integers: the recoded digits reconstruct the scalar through the split, every
pick lies inside the table, the scalar set of the GPU test reaches every entry under both signs, and the table walked on the CPU with the
one-lane host build of the kernels' point formulas gives the oracle's multiples of the generator."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from tests import gen_mul_cases as gc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("cpx_g1_generator_mul", "cpx_whisk_trackers_from_k_r")
KERNELS = ("k_gen_table", "k_gen_mul")
FR, AFF, JAC = 32, 96, 144


@pytest.fixture(scope="module")
def lib():
    from curdleproofs_amd.build import build
    build()
    import curdleproofs_amd as cpx
    return cpx.load_library()


@pytest.fixture(scope="module")
def emul():
    src = os.path.join(HERE, "host_emul", "gen_table_emul.cpp")
    so = os.path.join(HERE, "host_emul", "_gen_table.so")
    csrc = os.path.join(ROOT, "curdleproofs_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("gen_table.hpp", "glv.hpp", "g1_28.hpp", "fp28.hpp", "g1.hpp", "mont32.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.emul_gen_consts.argtypes = [vp]
    L.emul_gen_layout.argtypes = [vp, vp, vp]
    L.emul_gen_recode.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp]
    L.emul_gen_table_build.argtypes = [vp]
    L.emul_gen_table_entry.argtypes = [ctypes.c_int, vp]
    L.emul_gen_mul.argtypes = [ctypes.c_int, vp, vp, vp]
    for f in (L.emul_gen_consts, L.emul_gen_layout, L.emul_gen_recode, L.emul_gen_table_build, L.emul_gen_table_entry, L.emul_gen_mul):
        f.restype = None
    return L


@pytest.fixture(scope="module")
def consts(emul):
    c = (ctypes.c_int * 6)()
    emul.emul_gen_consts(c)
    return dict(zip(("windows", "digit_max", "top_digit_max", "entries", "max_adds", "entry_bytes"), c))


@pytest.fixture(scope="module")
def layout(emul, consts):
    n = consts["entries"]
    w, m, cap = (ctypes.c_int * n)(), (ctypes.c_int * n)(), (ctypes.c_int * consts["windows"])()
    emul.emul_gen_layout(w, m, cap)
    return list(w), list(m), list(cap)


def _recode(emul, consts, scalars):
    """per scalar: (neg_k, neg_t, |t|, q) and the picks {(half, window): (index, neg)}"""
    n, W = len(scalars), consts["windows"]
    halves = ctypes.create_string_buffer(32 * n)
    signs, index, neg = (ctypes.c_int * (2 * n))(), (ctypes.c_int * (2 * W * n))(), (ctypes.c_int * (2 * W * n))()
    emul.emul_gen_recode(n, gc.to_bytes(scalars), halves, signs, index, neg)
    out = []
    for c in range(n):
        t = int.from_bytes(halves.raw[32 * c:32 * c + 16], "little")
        q = int.from_bytes(halves.raw[32 * c + 16:32 * c + 32], "little")
        picks = {(h, w): (index[(2 * c + h) * W + w], neg[(2 * c + h) * W + w]) for h in (0, 1) for w in range(W)}
        out.append(((signs[2 * c], signs[2 * c + 1], t, q), picks))
    return out


def _random_scalars(count, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(gc.R_) for _ in range(count)]


# ---- the boundary ----
def test_header_declares_both_calls_beside_their_reference_lines():
    hdr = open(os.path.join(ROOT, "include", "cpx.h")).read()
    for name, cites in zip(NAMES, (("whisk.rs:318,323",), ("whisk.rs:45-55", "whisk.rs:370"))):
        at = hdr.index("int %s(" % name)
        comment = hdr[hdr.rindex("/*", 0, at):at]
        for cite in cites:
            assert cite in comment, "%s: %s is not cited beside the declaration" % (name, cite)
        assert comment.rstrip().endswith("*/")
    for k in KERNELS:
        assert '"%s"' % k in hdr, "cpx_get_stat's comment does not list %s" % k
    assert "NOT rejected" in hdr          # what a scalar >= r means is said in the header


def test_names_are_exported_everywhere(lib):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "whisk_mi355x.rs")).read()
    for name in NAMES:
        assert name in cpx.EXPORTS
        assert hasattr(lib, name), "libcpx.so does not export %s" % name
        assert re.search(r"pub fn %s\(" % name, ffi), "integration/rust/ffi.rs lacks %s" % name
        assert name + "(" in rs, "integration/rust/whisk_mi355x.rs does not call %s" % name
    for k in KERNELS:
        assert k in cpx.Context.KERNELS
    assert callable(cpx.Context.generator_mul) and callable(whisk.trackers_from_k_r) and callable(whisk.k_commitments)


def test_null_arguments_are_rejected_without_a_device(lib):
    import curdleproofs_amd as cpx
    buf = (ctypes.c_uint8 * 96)(*([0xaa] * 96))
    assert lib.cpx_g1_generator_mul(None, 1, None, buf, buf) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_trackers_from_k_r(None, 1, None, buf, buf, buf) == cpx.CPX_ERR_ARG
    assert lib.cpx_whisk_trackers_from_k_r(None, 1, buf, None, buf, buf) == cpx.CPX_ERR_ARG
    assert lib.cpx_g1_generator_mul(None, 1, buf, buf, buf) == cpx.CPX_ERR_ARG              # a NULL context
    assert lib.cpx_whisk_trackers_from_k_r(None, 1, buf, buf, buf, buf) == cpx.CPX_ERR_ARG
    assert bytes(buf) == b"\xaa" * 96                                                       # nothing was written


def test_python_wrappers_check_lengths_before_touching_the_library():
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    ctx = None                                             # any use of the context would raise AttributeError, not ValueError
    with pytest.raises(ValueError):
        whisk.trackers_from_k_r(ctx, [bytes(32)], [])
    with pytest.raises(ValueError):
        whisk.trackers_from_k_r(ctx, [bytes(31)], [bytes(32)])
    with pytest.raises(ValueError):
        whisk.k_commitments(ctx, [bytes(33)])
    with pytest.raises(ValueError):
        cpx.Context.generator_mul(ctx, bytes(33))
    assert whisk.trackers_from_k_r(ctx, [], []) == ([], []) and whisk.k_commitments(ctx, []) == []


# ---- gen_table.hpp against Python integers ----
def test_table_shape_is_what_the_halves_need(consts, layout):
    assert consts["windows"] == gc.WINDOWS == 16 and consts["digit_max"] == 128
    # the top digit's range follows from the sizes of the halves (|t| <= z^2 / 2, q <= round((r - 1) / 2 / z^2)): no carry window
    assert consts["top_digit_max"] == gc.top_digit_max() == 0x56
    assert consts["entries"] == 15 * 128 + 0x56 and consts["max_adds"] == 32
    assert consts["entries"] * consts["entry_bytes"] == 224672           # the bytes DESIGN.md states
    window, mult, cap = layout
    assert cap == [128] * 15 + [0x56]
    assert sorted(zip(window, mult)) == [(w, j) for w in range(16) for j in range(1, cap[w] + 1)]     # every multiple once, nothing else


def test_recoded_digits_reconstruct_the_scalar(emul, consts, layout):
    window, mult, _ = layout
    scalars = gc.edge_scalars() + gc.coverage_scalars() + _random_scalars(300, 20261017)
    for k, (halves, picks) in zip(scalars, _recode(emul, consts, scalars)):
        neg_k, neg_t, t, q = halves
        assert halves == gc.split(k), hex(k)                              # the twin's split against Python's
        assert ((-1) ** neg_k * ((-1) ** neg_t * t + q * gc.Z2) - k) % gc.R_ == 0
        total = 0
        for (h, w), (idx, neg) in picks.items():
            if idx < 0:
                continue
            assert 0 <= idx < consts["entries"] and window[idx] == w, (hex(k), h, w, idx)     # inside the table, in its own window
            total += (-1 if neg else 1) * mult[idx] * 256 ** w * (gc.Z2 if h else 1)
        assert (total - k) % gc.R_ == 0, hex(k)


def test_gpu_scalar_set_reaches_every_table_entry_under_both_signs(emul, consts, layout):
    window, mult, _ = layout
    scalars = gc.coverage_scalars()
    assert 1000 <= len(scalars) <= 4000
    seen = set()
    for k, (_, picks) in zip(scalars, _recode(emul, consts, scalars)):
        for (h, w), (idx, neg) in picks.items():
            if idx >= 0:
                seen.add((h, w, mult[idx], neg))
    want = gc.all_picks()
    assert len(want) == 2 * 2 * consts["entries"]
    assert seen == want, sorted(want - seen)[:8]


def test_edge_scalars_are_the_ones_the_issue_names():
    e = gc.edge_scalars()
    for v in (0, 1, 2, gc.R_ - 1, gc.R_ - 2, gc.Z2, gc.Z2 - 1, gc.Z2 + 1, gc.Z2 // 2, (gc.R_ + 1) // 2, (gc.R_ - 1) // 2, 2 ** 128 - 1, 2 ** 127,
              127, 128, 255, 256):
        assert v in e
    digits = [gc.signed_digits(gc.split(k)[2])[:-1] for k in e]
    assert [-128] + [-127] * 14 in digits and [127] * 15 in digits       # both ends of the digit range


def test_table_walk_on_the_cpu_matches_the_oracle(emul, consts, layout, orc):
    window, mult, _ = layout
    gen = orc.g1_generator()
    emul.emul_gen_table_build(gen)
    fr = lambda v: orc.fr_from_canonical_bytes((v % gc.R_).to_bytes(32, "little"))
    # the table itself: a sample of entries and the last one of every window
    sample = sorted(set(range(0, consts["entries"], 97)) | {e for e in range(consts["entries"]) if e + 1 == consts["entries"] or window[e + 1] != window[e]})
    want = orc.g1_scale(gen * len(sample), b"".join(fr(mult[e] * 256 ** window[e]) for e in sample))
    for i, e in enumerate(sample):
        out = ctypes.create_string_buffer(AFF)
        emul.emul_gen_table_entry(e, out)
        assert out.raw == want[AFF * i:AFF * (i + 1)], e
    # the walk: edge scalars, a slice of the coverage set, random ones
    scalars = gc.edge_scalars() + gc.coverage_scalars()[::7] + _random_scalars(64, 7)
    n = len(scalars)
    out = ctypes.create_string_buffer(JAC * n)
    adds = (ctypes.c_int * n)()
    emul.emul_gen_mul(n, gc.to_bytes(scalars), out, adds)
    got = orc.g1_compress_jac(out.raw)
    want = orc.g1_compress(orc.g1_scale(gen * n, b"".join(fr(k) for k in scalars)))
    for i, k in enumerate(scalars):
        assert got[48 * i:48 * (i + 1)] == want[48 * i:48 * (i + 1)], hex(k)
    assert got[:48] == bytes([0xc0]) + bytes(47) and adds[0] == 0        # the zero scalar: 32 additions of the identity
    assert max(adds) == consts["max_adds"] and adds[1] == 1
