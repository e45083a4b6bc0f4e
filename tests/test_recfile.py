"""fpx_recfile.hpp, the engine's one writer of Fortran unformatted sequential records (length, payload, length), compiled
as host code (tests/recfile_host.cpp): the bytes of its records against expectations built with struct, and what it
reports when a file cannot be opened or written."""
import os
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def rec(payload):
    return struct.pack("<i", len(payload)) + payload + struct.pack("<i", len(payload))


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("recfile_host")
    exe = d / "recfile_host"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(HERE, "recfile_host.cpp"), "-o", str(exe)])
    out = d / "out"
    out.mkdir()
    p = subprocess.run([str(exe), str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return out, p.stdout.splitlines()


def test_record_bytes(host_run):
    out, lines = host_run
    assert lines[0] == "written 1"
    read = lambda name: open(out / name, "rb").read()
    assert read("empty.bin") == rec(b"") == bytes(8)
    assert read("four.bin") == rec(struct.pack("<i", 3600))
    assert read("mixed.bin") == rec(struct.pack("<if", -999, 999.0)) + rec(struct.pack("<i", 5))
    assert read("reals.bin") == rec(struct.pack("<1000f", *(0.5 * i for i in range(1000))))
    # concoutput: the time, then per dump the four records count, indices, count, values -- for counts (0, 0) and (2, 5)
    want = rec(struct.pack("<i", 7200))
    want += rec(struct.pack("<i", 0)) + rec(b"") + rec(struct.pack("<i", 0)) + rec(b"")
    want += rec(struct.pack("<i", 2)) + rec(struct.pack("<2i", 33, 37)) + rec(struct.pack("<i", 5)) + rec(struct.pack("<5f", 1, 2, -3, 4, 5))
    assert read("conc.bin") == want
    assert read("plain.bin") == b"abcde"                       # write(): no markers; mode "ab" appends


def test_failures_are_reported(host_run):
    out, lines = host_run
    assert lines[1] == "nodir open=0 ok=0 close=0"
    assert sorted(os.listdir(out)) == ["conc.bin", "empty.bin", "four.bin", "mixed.bin", "plain.bin", "reals.bin"]   # nothing was written for it
    if os.path.exists("/dev/full"):
        assert lines[2] == "devfull close=0 again=0"           # the flush of fclose is where a full device shows
    else:
        assert lines[2] == "devfull absent"
