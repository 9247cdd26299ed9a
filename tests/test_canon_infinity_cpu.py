"""CPU checks of the infinity rewrite (curdleproofs_amd/csrc/canon_infinity.hpp) that Engine::canonical_infinities applies, under option
strict_infinity = 0, to every input of compressed points: run on the CPU by tests/host_emul/canon_infinity_emul.cpp, once plain and once
with -fsanitize=address,undefined, and compared with the rule stated in Python.  The store is the caller's: what one call returned is
still intact after the next call has rewritten another array into another store."""
import random
import subprocess

import pytest

from tests.check_harness import build_emul

CANON = bytes([0xc0]) + bytes(47)
# tests/test_gpu_parity.py, test_noncanonical_infinity_encodings_follow_the_option: sort flag set, the last bit of x, every bit, a high bit of x
VARIANTS = [bytes([0xe0]) + bytes(47), bytes([0xc0]) + bytes(46) + b"\x01", bytes([0xff]) + b"\xff" * 47, bytes([0xc0, 0x01]) + bytes(46)]
UNTOUCHED_STORE = b"store"      # what the twin fills every store with before the call


def rule(blob, nrec, stride, offsets):
    """An encoding whose first byte has both top bits set is the infinity; it is non-canonical unless it is 0xc0 followed by 47 zero bytes,
    and then it is replaced by that"""
    out = bytearray(blob)
    for r in range(nrec):
        for off in offsets:
            at = r * stride + off
            if out[at] & 0xc0 == 0xc0 and bytes(out[at:at + 48]) != CANON:
                out[at:at + 48] = CANON
    return bytes(out)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    exe = build_emul("canon_infinity_emul.cpp", ["canon_infinity.hpp"], request.param == "sanitized", hip=False)

    def run(arrays):
        """arrays: (blob, nrec, stride, offsets), each rewritten into a store of its own, one call after the other.  Returns per array
        (the returned pointer is the input, the bytes behind the returned pointer, the store) — all read after the LAST call."""
        text = "%d\n" % len(arrays)
        for blob, nrec, stride, offsets in arrays:
            assert len(blob) == nrec * stride
            text += "%d %d %d %s\n%s\n" % (nrec, stride, len(offsets), " ".join(str(o) for o in offsets), blob.hex() or "-")
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()   # a sanitizer report is a non-zero exit
        assert len(out) == 3 * len(arrays)
        res = []
        unhex = lambda s: b"" if s == "-" else bytes.fromhex(s)
        for a in range(len(arrays)):
            same, got = out[3 * a].split()
            tag, store = out[3 * a + 1].split()
            assert same in ("0", "1") and tag == "STORE" and out[3 * a + 2] == "INPUT 1"       # the input is never written
            res.append((same == "1", unhex(got), unhex(store)))
        return res
    return run


def check(emul, blob, nrec, stride, offsets):
    (same, got, store), = emul([(blob, nrec, stride, offsets)])
    want = rule(blob, nrec, stride, offsets)
    assert got == want
    assert same == (want == blob)                                # no rewrite: the input itself comes back ...
    assert store == (UNTOUCHED_STORE if same else want)          # ... and the store is left as it was; otherwise the store is the result
    return same


def records(rnd, nrec, stride):
    """random bytes whose encodings at offsets 0 and 48 are no infinities (the top bits of their first byte are 10: compressed, finite)"""
    blob = bytearray(rnd.randbytes(nrec * stride))
    for r in range(nrec):
        for off in (0, 48):
            if off + 48 <= stride:
                blob[r * stride + off] = 0x80 | (blob[r * stride + off] & 0x3f)
    return blob


LAYOUTS = [(48, (0,)), (96, (0, 48)), (128, (0, 48)), (48 + 80, (0,))]


@pytest.mark.parametrize("stride,offsets", LAYOUTS)
def test_nothing_to_rewrite_returns_the_input_and_leaves_the_store(emul, stride, offsets):
    rnd = random.Random(stride * 7 + len(offsets))
    for nrec in (0, 1, 5):
        blob = records(rnd, nrec, stride)
        for r in range(nrec):                                  # the canonical infinity is no rewrite either
            if r % 2:
                blob[r * stride + offsets[-1]:r * stride + offsets[-1] + 48] = CANON
        assert check(emul, bytes(blob), nrec, stride, offsets) is True


@pytest.mark.parametrize("stride,offsets", LAYOUTS)
@pytest.mark.parametrize("nrec", (1, 2, 9))
def test_every_variant_at_the_first_and_the_last_record(emul, nrec, stride, offsets):
    rnd = random.Random(1000 * nrec + stride)
    for v in VARIANTS:
        for r in sorted({0, nrec - 1}):
            for off in offsets:
                blob = records(rnd, nrec, stride)
                blob[r * stride + off:r * stride + off + 48] = v
                assert check(emul, bytes(blob), nrec, stride, offsets) is False
    blob = records(rnd, nrec, stride)                          # every encoding of every record at once, the variants in turn
    for r in range(nrec):
        for i, off in enumerate(offsets):
            blob[r * stride + off:r * stride + off + 48] = VARIANTS[(r + i) % len(VARIANTS)]
    assert check(emul, bytes(blob), nrec, stride, offsets) is False


def test_bytes_behind_the_listed_offsets_stay_untouched(emul):
    """stride 48 + 80 with offset 0 only (a proof record: M, then bytes that are not this call's): what looks like a flag at byte 48, or
    anywhere behind the first encoding, is left alone — alone it causes no copy, and beside a rewrite it is copied as it is"""
    stride, nrec = 48 + 80, 3
    rnd = random.Random(5)
    blob = records(rnd, nrec, stride)
    for r in range(nrec):
        blob[r * stride + 48:r * stride + 96] = VARIANTS[r % len(VARIANTS)]
        blob[r * stride + 96] = 0xff
    assert check(emul, bytes(blob), nrec, stride, (0,)) is True
    blob[2 * stride:2 * stride + 48] = VARIANTS[2]
    (same, got, _), = emul([(bytes(blob), nrec, stride, (0,))])
    assert not same and got == bytes(blob[:2 * stride]) + CANON + bytes(blob[2 * stride + 48:])
    assert check(emul, bytes(blob), nrec, stride, (0, 48)) is False      # ... and with both offsets listed, both are rewritten


def test_two_arrays_one_after_the_other_keep_their_results(emul):
    """three arrays of one call, the middle one without a rewrite: every result is read after the last call and is still what the rule says"""
    rnd = random.Random(11)
    a = records(rnd, 4, 96)
    a[96 + 48:96 + 96] = VARIANTS[0]
    b = records(rnd, 4, 48)
    c = records(rnd, 4, 128)
    c[3 * 128:3 * 128 + 48] = VARIANTS[1]
    arrays = [(bytes(a), 4, 96, (0, 48)), (bytes(b), 4, 48, (0,)), (bytes(c), 4, 128, (0, 48))]
    res = emul(arrays)
    for (blob, nrec, stride, offsets), (same, got, store) in zip(arrays, res):
        assert got == rule(blob, nrec, stride, offsets)
        assert same == (got == blob) and store == (UNTOUCHED_STORE if same else got)
    assert [same for same, _, _ in res] == [False, True, False]
