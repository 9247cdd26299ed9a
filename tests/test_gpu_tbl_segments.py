"""Two-segment per-proof tables (option tbl_segments, curdleproofs_amd/csrc/kernels.h "table-backed MSM"): 8 + 8 shifted copies per base
instead of 16 + 16, the windows 8..15 of an endomorphism half in a weight class of their own whose sum is doubled 64 times per MSM
output.  The proofs are the same group elements under either layout: every case runs tbl_segments = 1 and 2, requires the oracle's
bytes, and checks that `tbl_segments_effective` reports the layout the batch's path supports — two segments on the device-resident
prover whose SameMSM rounds are not fused launches (stand-alone bucket-list waves, k_late_uniform), one segment on the fused rounds
(round.hip), the lone-proof kernels and the host-driven prover."""
import pytest

from tests import test_gpu_parity as parity   # (its checks are called through the module: imported by name they would be collected again here)
from tests.test_gpu_parity import THROUGHPUT, _prove_and_check, _variant_checks

pytestmark = pytest.mark.gpu


def _expected(c, nproofs, ell):
    """Engine::tbl_segments_for (engine.cpp), from the context's options."""
    g = c.get_option
    n = ell + 4
    L = n.bit_length() - 1
    want = g("tbl_segments") or (2 if n <= 256 else 1)
    if want != 2 or nproofs < g("device_min_batch"):
        return 1
    supported = lambda m: 2 <= m <= 64 and n % m == 0 and n // m <= 128 and n > m
    m = g("late_m") or (32 if n >= 512 else 16)
    while m > 16 and not supported(m):
        m //= 2
    late_min = g("late_min_batch") if n <= 256 else max(1, g("late_min_batch") * 256 // n)
    late_on = g("late_rounds") != 0 and L >= m.bit_length() and nproofs >= late_min and supported(m)
    fused_max = g("fused_smsm_max") if n <= 256 else g("fused_smsm_max") * 256 // n
    may_fuse = not late_on and g("fix_bits_effective") == 16 and not g("serial_streams") and g("fused_smsm_max") > 0 and nproofs <= fused_max
    return 1 if may_fuse else 2


def _watched(options):
    """A context whose every prove checks tbl_segments_effective against _expected; .seen collects the layouts that ran."""
    import curdleproofs_amd as cpx
    c = cpx.Context(0, options=options)
    c.seen = set()
    state = {}
    plain_set_crs, plain_prove = c.set_crs, c.prove_batch

    def set_crs(ell, pts):
        state["ell"] = ell
        return plain_set_crs(ell, pts)

    def prove_batch(*a, **k):
        proofs = plain_prove(*a, **k)
        eff = c.get_option("tbl_segments_effective")
        assert eff == _expected(c, len(proofs), state["ell"])
        c.seen.add(eff)
        return proofs

    c.set_crs, c.prove_batch = set_crs, prove_batch
    return c


UNFUSED = {"device_min_batch": 1, "fused_rounds_max": 0, "fused_smsm_max": 0}   # every round the chain of separate kernels, also for a few proofs
OPTION_SETS = {
    # (the SameMSM rounds of a small batch stay fused launches, hence one segment — unless the fixed-base table fell back from 16 bits, which
    # switches the fused rounds off: no fixed set of layouts to expect)
    "unfused_ipa_rounds": ({"device_min_batch": 1, "fused_rounds_max": 0}, None),
    "late_rounds_two_lanes_per_output": ({"device_min_batch": 1, "late_min_batch": 1}, {2}),
    "host_driven": ({"device_min_batch": 1000000}, {1}),
    "defaults": ({}, {1}),                                                         # (batches below device_min_batch: host-driven)
    "standalone_table_waves_and_tails": (UNFUSED, {2}),
}


@pytest.mark.parametrize("segments", [1, 2])
@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_variant_checks_under_both_layouts(name, segments, orc, whisk_kat, oracle_vectors):
    options, with_two = OPTION_SETS[name]
    c = _watched(dict(options, tbl_segments=segments))
    try:
        _variant_checks(c, orc, whisk_kat, oracle_vectors)
        if with_two is not None:
            assert c.seen == (with_two if segments == 2 else {1})
    finally:
        c.close()


LATE = {"device_min_batch": 1, "late_min_batch": 1}
SHAPES = {
    "ell28_two_points_per_materialised_base": (28, [0, 1, 2], LATE),        # a class of a magnitude can be empty
    "ell252_one_lane_per_output": (252, [0], dict(LATE, late_m=32)),        # the classes in sequence
    "ell508": (508, [0], LATE),                                            # default m = 32
    "ell252_all_msm_rounds": (252, [0], dict(UNFUSED, late_rounds=0)),
    # the throughput instantiations on a few proofs: 32 windows per wave (both classes in one wave, four raw sets), the thread-per-group
    # reductions and the thread-per-request finalisation that doubles the class-1 partial sums
    "ell28_throughput_kernels": (28, [0, 1, 2], dict(THROUGHPUT, **UNFUSED)),
    "ell252_throughput_kernels": (252, [0], dict(THROUGHPUT, **UNFUSED)),
    "ell252_sixteen_windows_per_wave_late": (252, [0], dict(LATE, tbw_wpw=16, reduce_wave_max=0, finalize_wave_max=0)),
}


@pytest.mark.parametrize("segments", [1, 2])
@pytest.mark.parametrize("name", list(SHAPES))
def test_proofs_match_oracle_under_both_layouts(name, segments, orc):
    ell, seeds, options = SHAPES[name]
    c = _watched(dict(options, tbl_segments=segments))
    try:
        _prove_and_check(c, orc, ell, seeds)
        assert c.seen == {segments}
    finally:
        c.close()


@pytest.mark.parametrize("segments", [1, 2])
@pytest.mark.parametrize("options", [{"tbw_wpw": w} for w in (2, 4, 8, 16, 32)] + [{"tbw_slices": s} for s in (2, 4)], ids=lambda o: "%s_%d" % next(iter(o.items())))
def test_window_groupings_and_slices_reproduce_kat_under_both_layouts(options, segments, orc, whisk_kat):
    # the device-resident chain of separate kernels, so that the pinned grouping reads the two-segment tables: waves of 2 / 4 / 8
    # windows lie inside one class, waves of 16 / 32 serve both.  (The point slices are the host-driven lone proof's: one segment.)
    sliced = "tbw_slices" in options
    c = _watched(dict(options if sliced else dict(UNFUSED, **options), tbl_segments=segments))
    try:
        parity.test_prove_matches_reference_kat_ell124(c, orc, whisk_kat)
        assert c.seen == {1 if sliced else segments}
    finally:
        c.close()


@pytest.mark.parametrize("options", [LATE, UNFUSED], ids=["late_rounds", "all_msm_rounds"])
def test_identity_and_repeated_points_on_two_segment_tables(options, orc):
    c = _watched(dict(options, tbl_segments=2))
    try:
        parity.test_instances_with_identity_points_and_repeated_points(c, orc, 97)
        assert c.seen == {2}
    finally:
        c.close()


def test_one_context_switches_layouts_between_two_proves_of_a_batch(orc):
    ell = 28
    c = _watched(LATE)
    try:
        c.set_profiling(True)
        crs = orc.generate_crs_points(ell)
        c.set_crs(ell, crs)
        insts = [orc.make_instance(ell, s, crs) for s in range(100, 140)]
        cat = lambda key: b"".join(i[key] for i in insts)
        c.load_batch(cat("vec_R"), cat("vec_S"), cat("vec_T"), cat("vec_U"), cat("M"))
        perms = [x for i in insts for x in i["permutation"]]
        runs = {}
        for segments in (1, 2, 1):
            c.set_option("tbl_segments", segments)
            c.reset_stats()
            runs.setdefault(segments, []).append(c.prove_batch(perms, cat("k"), cat("vec_m_blinders"), cat("prover_rand")))
            assert c.get_option("tbl_segments_effective") == segments
            assert c.stat("k_table_build")["launches"] > 0
        assert runs[1][0] == runs[2][0] == runs[1][1] == [i["proof"] for i in insts]
    finally:
        c.close()
