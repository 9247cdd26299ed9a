"""The record loop shared by the check programs (tests/device/check_harness.hpp) and its Python side (tests/check_harness.py), through
the five host twins: what a bad record, a missing file and a good record do is the same in every program."""
import struct
import subprocess

import numpy as np
import pytest

from tests import check_harness as ch
from tests import field_check_lib, rng_cases, rng_g1_cases, scalar_check_lib, transcript_cases

# program -> (library, its table as --list prints it, the payload of one valid row of the first table entry)
EMPTY_CASE = struct.pack("<4I27Q", 0, 0, 0, 0, *([0] * 27))      # transcript_check's strobe_host: no operation, no blob, a zero state
PROGRAMS = {"field": (field_check_lib, field_check_lib.TABLE, None), "scalar": (scalar_check_lib, scalar_check_lib.TABLE, None),
            "transcript": (transcript_cases, transcript_cases.HOST_TABLE, EMPTY_CASE), "rng": (rng_cases, rng_cases.TABLE, None),
            "rng_g1": (rng_g1_cases, rng_g1_cases.TABLE, None)}


@pytest.fixture(scope="module", params=list(PROGRAMS))
def program(request, tmp_path_factory):
    lib, table, payload = PROGRAMS[request.param]
    name, (ni, _) = next(iter(table.items()))
    exe = lib.build_host_twin(tmp_path_factory.mktemp(request.param), extra=["-O0"])      # (the loop is under test, not the arithmetic: a quick compile)
    return request.param + "_check", exe, name, ni, payload or bytes(4 * ni)


def _run(exe, tmp_path, tag, blob):
    inp, outp = tmp_path / (tag + ".in"), tmp_path / (tag + ".out")
    if blob is not None:
        inp.write_bytes(blob)
    r = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    return r, outp


def test_bad_records_exit_3_and_leave_no_output_record(program, tmp_path):
    prog, exe, name, ni, payload = program
    good = ch.pack_record(name, ni, 1, payload)
    for tag, blob in (("unknown", ch.pack_record("no_such_operation", ni, 1, payload)),
                      ("width", ch.pack_record(name, ni + 1, 1, payload + bytes(4))),
                      ("truncated", good[:-4]),
                      ("tail", good + bytes(5))):
        r, outp = _run(exe, tmp_path, tag, blob)
        assert r.returncode == 3 and prog + ":" in r.stderr, (tag, r.returncode, r.stderr)
        assert ch.read_records(str(outp)) == [], tag


def test_a_missing_input_exits_2(program, tmp_path):
    prog, exe, _, _, _ = program
    r, _ = _run(exe, tmp_path, "missing", None)
    assert r.returncode == 2 and prog + ": cannot open" in r.stderr


def test_one_valid_row(program, tmp_path):
    prog, exe, name, ni, payload = program
    r, outp = _run(exe, tmp_path, "one", ch.pack_record(name, ni, 1, payload))
    assert r.returncode == 0 and prog + " (host): 1 records, 1 rows" in r.stdout, r.stdout + r.stderr
    assert len(outp.read_bytes()) > 64


def test_words_round_trip_through_the_record_file(tmp_path):
    path = str(tmp_path / "words")
    ch.write_records(path, {"w": (4, 4)}, [("w", [[-1, -(1 << 31), (1 << 32) - 1, 0]])])
    (name, a), = ch.read_records(path)
    assert name == "w" and a.dtype == np.dtype("<u4") and a.tolist() == [[0xffffffff, 0x80000000, 0xffffffff, 0]]
    for bad in (-(1 << 31) - 1, 1 << 32):
        with pytest.raises(AssertionError):
            ch.write_records(path, {"w": (1, 1)}, [("w", [[bad]])])
