"""The binary database file (csrc/sw_dbfile.cpp) on the CPU, linked from that
file alone.  tests/native/dbfile_check.cpp writes and reads small files
(with an empty subject, with no subject) and hands read() files that are cut
inside each section, altered by one byte in each section, or not of this
format; the codes and messages are those sw_db_load reports through the CLI
(tests/test_gpu_cli.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SW_E_IO = -6  # include/sw_amd.h


@pytest.fixture(scope="module")
def dbfile_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dbfile")
    exe = str(tmp / "dbfile_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "dbfile_check.cpp"),
                    os.path.join(CSRC, "sw_dbfile.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, str(tmp)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("dbfile_check ok"), r.stdout + r.stderr
    # (a refusal's line ends where the message names the file)
    return dict(line.rstrip().split(": ", 1) for line in r.stdout.splitlines() if ": " in line.rstrip())


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_round_trip(dbfile_check):
    assert dbfile_check["round-trip"] == "3 subjects, 92 bytes"
    assert dbfile_check["round-trip-empty"] == "0 subjects, 48 bytes"


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_corrupt_files_are_refused(dbfile_check):
    io = "%d " % SW_E_IO
    for cut in ("offsets", "ids", "residues"):
        assert dbfile_check["cut-in-" + cut] == io + "truncated database file:"
    assert dbfile_check["cut-at-residues"] == io + "truncated database file:"
    # a file shorter than its header was never "truncated" to sw_db_load: it
    # cannot tell such a file from one of another format
    assert dbfile_check["cut-in-header"] == io + "not a database file (sw_db_save format 1):"
    for flip in ("offsets", "ids", "residues", "checksum"):
        assert dbfile_check["flip-in-" + flip] == io + "database file checksum mismatch:"
    for what in ("bad-magic", "version-2", "negative-n", "negative-residues", "empty-file"):
        assert dbfile_check[what] == io + "not a database file (sw_db_save format 1):"
    assert dbfile_check["residues-disagree-with-offsets"] == io + "database file checksum mismatch:"
