"""GPU parity of cpx_whisk_find_trackers (curdleproofs_amd.whisk.find_trackers): which key opens which tracker, k * r_G == k_r_G
(whisk.rs:36-55).  Every expected owner comes from the oracle — orc.g1_scale for every (tracker, key) pair, compared as compressed bytes —
and every expected decoding verdict from tests/decoding_ref.py; nothing comes from the library under test.  Sizes are the smallest that
cross the 64-column block of a scan wave (70 trackers: one full block and a 6-lane one) and a chunk boundary (9 trackers under a budget
of 1 - 3 MiB)."""
import ctypes

import pytest

from tests import find_cases as fc

pytestmark = pytest.mark.gpu

R_ = fc.R_
NEVER_TABLE = (1 << 20) + 1
PATHS = {"table": 1, "ladder": NEVER_TABLE}            # option find_table_min_keys
IDENTITY = bytes([0xc0]) + bytes(47)
N, NK = 70, 5
# trackers of the 70 x 5 batch with something special about them
R_ONE, NEGATED, SWAPPED, BOTH_IDENTITY, R_IDENTITY_ONLY, NONCANONICAL_R, NONCANONICAL_S = 3, 9, 39, 15, 16, 21, 22
DEFECTS = ("x not on the curve", "x >= p", "no compression flag", "outside the subgroup")
DEFECT_ON_R = dict(zip(DEFECTS, (27, 33, 40, 64)))      # ... on the r_G half (64: the first lane of the second column block)
DEFECT_ON_S = dict(zip(DEFECTS, (28, 34, 41, 69)))      # ... on the k_r_G half (69: the last live lane)


def _fr(orc, v):
    return orc.fr_from_canonical_bytes((v % R_).to_bytes(32, "little"))


def _flip_sort(enc):
    return bytes([enc[0] ^ 0x20]) + enc[1:]


def _expected(orc, trackers, keys_wire, strict):
    """(owners, ok) for 96-byte trackers and wire keys: decoding by tests/decoding_ref.py, every pair by the oracle's scalar multiplication"""
    from tests import decoding_ref as dr
    n = len(trackers)
    dec = [(dr.expected_output(t[:48], orc, bool(strict), True), dr.expected_output(t[48:], orc, bool(strict), True)) for t in trackers]
    ok = [a[0] == 0 and b[0] == 0 for a, b in dec]
    r_g = b"".join(a[1] for a, _ in dec)
    claimed = orc.g1_compress(b"".join(b[1] for _, b in dec))
    owners = [None] * n
    for j in reversed(range(len(keys_wire))):          # (descending: the smallest matching index is written last)
        prod = orc.g1_compress(orc.g1_scale(r_g, keys_wire[j]))
        for i in range(n):
            if ok[i] and prod[48 * i:48 * (i + 1)] == claimed[48 * i:48 * (i + 1)]:
                owners[i] = j
    return owners, ok


def _plant(orc, seed, n, keys_wire, planted):
    """n trackers with seeded r; planted[i] = index of the key that opens tracker i, or None for a k no key of the set equals"""
    from curdleproofs_amd import whisk
    rng = orc.rng(seed)
    rs = [rng.fr(1) for _ in range(n)]
    stray = rng.fr(1)
    gen = orc.g1_generator()
    r_g = orc.g1_scale(gen * n, b"".join(rs))
    k_r_g = orc.g1_scale(r_g, b"".join(stray if p is None else keys_wire[p] for p in planted))
    cr, ck = orc.g1_compress(r_g), orc.g1_compress(k_r_g)
    return [whisk.WhiskTracker(cr[48 * i:48 * (i + 1)], ck[48 * i:48 * (i + 1)]) for i in range(n)]


class Batch:
    """70 trackers x 5 keys: keys 0, 1, r - 1, a random one, and r - 1 again"""

    def __init__(self, orc):
        from curdleproofs_amd import whisk
        from tests import decoding_ref as dr
        self.keys = [_fr(orc, 0), _fr(orc, 1), _fr(orc, R_ - 1), orc.rng(77).fr(1), _fr(orc, R_ - 1)]
        planted = [(None if i % 6 == 5 else i % 6) for i in range(N)]             # spread over the keys; every sixth tracker is nobody's
        t = _plant(orc, 4242, N, self.keys, planted)
        gen = orc.g1_compress(orc.g1_generator())
        t[R_ONE] = whisk.WhiskTracker(gen, orc.g1_compress(orc.g1_scale(orc.g1_generator(), self.keys[3])))     # r = 1: r_G = G
        assert planted[NEGATED] == 3 and planted[SWAPPED] == 3                    # the random key (under k = r - 1 swapped halves still match)
        t[NEGATED] = whisk.WhiskTracker(t[NEGATED].r_G, _flip_sort(t[NEGATED].k_r_G))
        t[SWAPPED] = whisk.WhiskTracker(t[SWAPPED].k_r_G, t[SWAPPED].r_G)
        t[BOTH_IDENTITY] = whisk.WhiskTracker(IDENTITY, IDENTITY)
        t[R_IDENTITY_ONLY] = whisk.WhiskTracker(IDENTITY, t[R_IDENTITY_ONLY].k_r_G)
        noncanonical = bytes([0xc0]) + bytes(46) + b"\x01"
        t[NONCANONICAL_R] = whisk.WhiskTracker(noncanonical, IDENTITY)           # strict_infinity = 0: the identity twice, owner 0
        t[NONCANONICAL_S] = whisk.WhiskTracker(t[NONCANONICAL_S].r_G, noncanonical)
        bad = {"x not on the curve": dr.encode(dr.off_curve_xs(1)[0], 0x80), "x >= p": dr.encode(dr.P + 1, 0x80),
               "no compression flag": bytes([t[0].r_G[0] & 0x7f]) + t[0].r_G[1:], "outside the subgroup": dr.compress(dr.non_member_points(orc, 1)[0])}
        assert dr.decode(bad["outside the subgroup"], orc)[0] == dr.NOT_IN_SUBGROUP and all(dr.decode(b, orc)[0] != dr.OK for b in bad.values())
        for name in DEFECTS:
            i, j = DEFECT_ON_R[name], DEFECT_ON_S[name]
            t[i] = whisk.WhiskTracker(bad[name], t[i].k_r_G)
            t[j] = whisk.WhiskTracker(t[j].r_G, bad[name])
        self.trackers = t
        self.want = {s: _expected(orc, [x.to_bytes() for x in t], self.keys, s) for s in (0, 1)}
        # what the oracle says about the special trackers: every kind of answer is present
        own, ok = self.want[0]
        assert own[R_ONE] == 3 and own[NEGATED] is None and own[SWAPPED] is None and own[BOTH_IDENTITY] == 0 and own[R_IDENTITY_ONLY] is None
        assert own[NONCANONICAL_R] == 0 and ok[NONCANONICAL_R] and ok[NONCANONICAL_S]
        assert [i for i in range(N) if not ok[i]] == sorted(list(DEFECT_ON_R.values()) + list(DEFECT_ON_S.values()))
        assert own[4] == 2 and planted[4] == 4                                    # key 4 equals key 2: the smaller index
        assert {own[i] for i in range(N)} == {None, 0, 1, 2, 3}
        own1, ok1 = self.want[1]
        assert not ok1[NONCANONICAL_R] and not ok1[NONCANONICAL_S] and own1[NONCANONICAL_R] is None
        assert [i for i in range(N) if ok[i] != ok1[i]] == [NONCANONICAL_R, NONCANONICAL_S]


@pytest.fixture(scope="module")
def batch(orc):
    return Batch(orc)


def _ctx(**options):
    import curdleproofs_amd as cpx
    return cpx.Context(0, options=options)


def _answers(result):
    """whisk.find_trackers' (owners, status) -> (owners, ok flags), with the return types checked"""
    from curdleproofs_amd import whisk
    owners, status = result
    assert len(owners) == len(status)
    for o, s in zip(owners, status):
        assert o is None or type(o) is int
        assert s is True or isinstance(s, whisk.SerializationError)
        assert s is True or o is None
    return owners, [s is True for s in status]


@pytest.mark.parametrize("strict", [0, 1], ids=["ark_0_4_infinity", "strict_infinity"])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_owners_match_the_oracle_on_both_paths(batch, path, strict):
    from curdleproofs_amd import whisk
    c = _ctx(find_table_min_keys=PATHS[path], strict_infinity=strict)
    try:
        got = _answers(whisk.find_trackers(c, batch.trackers, batch.keys))
    finally:
        c.close()
    want = batch.want[strict]
    assert got[1] == want[1], [i for i in range(N) if got[1][i] != want[1][i]]
    assert got[0] == want[0], [(i, g, w) for i, (g, w) in enumerate(zip(got[0], want[0])) if g != w]


def test_chunked_scan_agrees_with_one_chunk_and_the_oracle(orc):
    """9 trackers x 64 keys; find_table_mb = 1 holds one column per chunk (nine chunks), 3 holds five (chunks of 5 and 4)"""
    from curdleproofs_amd import whisk
    rng = orc.rng(99)
    keys = [rng.fr(1) for _ in range(64)]
    planted = [0, 63, 17, None, 32, 5, 63, 40, 1]
    trackers = _plant(orc, 5150, 9, keys, planted)
    want = _expected(orc, [t.to_bytes() for t in trackers], keys, 0)
    assert want == (planted, [True] * 9)
    got = {}
    for mb in (1, 3, 1024):
        c = _ctx(find_table_mb=mb, find_table_min_keys=1)
        try:
            c.set_profiling(True)
            got[mb] = _answers(whisk.find_trackers(c, trackers, keys))
            assert c.stat("k_find_scan")["launches"] == {1: 9, 3: 2, 1024: 1}[mb]     # one scan per chunk
            assert c.stat("k_find_scan")["units"] == 9 * 64
        finally:
            c.close()
    assert got[1] == got[3] == got[1024] == want


def test_every_table_pick(orc):
    """one tracker per key of the coverage and edge sets: every (window, magnitude, sign) a reduced key can ask of the table is walked, and
    tracker i is opened by key i alone"""
    from curdleproofs_amd import whisk
    cov = fc.coverage_keys()
    ints = cov + [k for k in fc.edge_keys() if k not in set(cov)]
    assert len(set(k % R_ for k in ints)) == len(ints) and 256 < len(ints) < 400       # distinct mod r
    assert fc.picks_of(ints) == fc.attainable_picks()
    keys = [_fr(orc, k) for k in ints]
    n = len(keys)
    trackers = _plant(orc, 8086, n, keys, list(range(n)))
    c = _ctx(find_table_min_keys=1)
    try:
        owners, ok = _answers(whisk.find_trackers(c, trackers, keys))
    finally:
        c.close()
    assert ok == [True] * n
    assert owners == list(range(n)), [(i, o, hex(ints[i])) for i, o in enumerate(owners) if o != i][:8]


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("n,nk", [(1, 1), (63, 1), (64, 1), (65, 2)])
def test_shape_edges(batch, orc, path, n, nk):
    from curdleproofs_amd import whisk
    trackers, keys = batch.trackers[:n], batch.keys[3:3 + nk]                      # the random key, then r - 1
    want = _expected(orc, [t.to_bytes() for t in trackers], keys, 0)
    c = _ctx(find_table_min_keys=PATHS[path])
    try:
        assert _answers(whisk.find_trackers(c, trackers, keys)) == want
    finally:
        c.close()
    assert any(o is not None for o in want[0]) or n == 1


def test_no_keys_no_trackers_and_null_arguments(batch):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    c = _ctx()
    try:
        owners, ok = _answers(whisk.find_trackers(c, batch.trackers, []))          # still decoded, nobody's
        assert owners == [None] * N and ok == batch.want[0][1]
        assert whisk.find_trackers(c, [], batch.keys) == ([], [])
        f = c._L.cpx_whisk_find_trackers
        owner, status = (ctypes.c_uint32 * 2)(7, 7), (ctypes.c_int * 2)(55, 55)
        blob = cpx._in(b"".join(t.to_bytes() for t in batch.trackers[2:4]))     # key 3 opens the second of them (R_ONE)
        key = cpx._in(batch.keys[3])
        assert f(c._h, 0, None, 0, None, None, None) == cpx.CPX_OK                  # n_trackers = 0: a no-op
        assert f(c._h, 0, None, 1, key, owner, status) == cpx.CPX_OK and list(owner) == [7, 7] and list(status) == [55, 55]
        assert f(c._h, 2, None, 1, key, owner, status) == cpx.CPX_ERR_ARG
        assert f(c._h, 2, blob, 1, None, owner, status) == cpx.CPX_ERR_ARG
        assert f(c._h, 2, blob, 1, key, None, status) == cpx.CPX_ERR_ARG
        assert f(c._h, 2, blob, 1, key, owner, None) == cpx.CPX_ERR_ARG
        assert f(c._h, (1 << 23) + 1, blob, 1, key, owner, status) == cpx.CPX_ERR_ARG
        assert list(owner) == [7, 7] and list(status) == [55, 55]                  # nothing was written
        assert f(c._h, 2, blob, 0, None, owner, status) == cpx.CPX_OK              # no keys: k may be NULL
        assert list(owner) == [cpx.CPX_NO_OWNER] * 2 and list(status) == [cpx.CPX_OK] * 2
        assert f(c._h, 2, blob, 1, key, owner, status) == cpx.CPX_OK
        assert list(owner) == [cpx.CPX_NO_OWNER, 0] and list(status) == [cpx.CPX_OK] * 2 and batch.want[0][0][2:4] == [2, 3]
    finally:
        c.close()


def test_loaded_batch_and_crs_are_left_alone(batch, orc):
    import curdleproofs_amd as cpx
    from curdleproofs_amd import whisk
    ell = 28
    crs = orc.generate_crs_points(ell)
    inst = orc.make_instance(ell, 0, crs)
    for path in sorted(PATHS):
        c = _ctx(find_table_min_keys=PATHS[path])
        try:
            c.set_crs(ell, crs)
            c.load_batch(*(inst[k] * 2 for k in ("vec_R", "vec_S", "vec_T", "vec_U", "M")))
            before = c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2)
            assert c.batch == 2 and before == [cpx.CPX_OK] * 2
            assert _answers(whisk.find_trackers(c, batch.trackers, batch.keys)) == batch.want[0]
            assert c.batch == 2
            assert c.verify_batch([inst["proof"]] * 2, inst["verifier_rand"] * 2) == before
            assert c.crs_sums() == orc.crs_sums(ell, crs)
        finally:
            c.close()
    # (a context without a CRS: every other test of this file)


def test_which_kernels_ran(batch):
    from curdleproofs_amd import whisk
    names = ("k_decompress", "k_table_build", "k_fix_build", "k_find_scan", "k_smul", "k_find_compare")
    seen = {}
    for path in sorted(PATHS):
        c = _ctx(find_table_min_keys=PATHS[path])
        try:
            c.set_profiling(True)
            for count in (9, N):
                c.reset_stats()
                whisk.find_trackers(c, batch.trackers[:count], batch.keys)
                seen[path, count] = {k: c.stat(k)["launches"] for k in names}
            c.reset_stats()
            whisk.find_trackers(c, batch.trackers, batch.keys[:2])
            seen[path, "two keys"] = {k: c.stat(k)["launches"] for k in names}
        finally:
            c.close()
    table = {"k_decompress": 1, "k_table_build": 1, "k_fix_build": 1, "k_find_scan": 1, "k_smul": 0, "k_find_compare": 0}
    ladder = {"k_decompress": 1, "k_table_build": 0, "k_fix_build": 0, "k_find_scan": 0, "k_smul": 1, "k_find_compare": 1}
    for what in (9, N, "two keys"):                        # never per tracker, never per key
        assert seen["table", what] == table, what
        assert seen["ladder", what] == ladder, what
