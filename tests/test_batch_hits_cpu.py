"""CPU: the batched hit table's pure pieces.  tests/native/batch_hits_check.cpp
pins swplan::hits_cost to the bounds of the kernel's own loops, hits_order to
a stable descending permutation and the per-hit hits_groups to the budget, to
greedy closing and to the single-qlen form.  The CLI's --queries checks run
before any file is read, and tests/native/read_queries_check.cpp prints what
sw_solver_read_queries makes of a file: neither needs a GPU.

hits_cost counts rounds of 64 steps, and lane 63 ends a subject of L columns
at step L + 62: a block is added at L = 2, 66, 130, ... (not at 65), which is
where the native check looks for the step."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "csrc")
LIB = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "lib")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INC = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]

needs_hipcc = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


@pytest.fixture(scope="module")
def batch_hits_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("batch_hits")
    objs = []
    for src in (os.path.join(ROOT, "tests", "native", "batch_hits_check.cpp"), os.path.join(CSRC, "sw_plan.cpp")):
        objs.append(str(tmp / (os.path.basename(src) + ".o")))
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall"] + INC + ["-c", src, "-o", objs[-1]],
                       check=True, timeout=300)
    exe = str(tmp / "batch_hits_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950"] + objs + ["-o", exe, "-lpthread"], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("batch_hits_check ok"), r.stdout[-4000:] + r.stderr[-2000:]
    return r.stdout


@needs_hipcc
def test_cost_follows_the_kernels_loops(batch_hits_check):
    m = re.search(r"cost: C (\d+) rounds at slen 100, C\+1 (\d+), steps in slen 1\.\.400 (\d+)", batch_hits_check)
    assert m, batch_hits_check
    c, c1, steps = map(int, m.groups())
    # slen 100: 3 blocks; a full chunk adds 2 rounds for each of the 3 further waves; C + 1 a chunk of one wave
    assert c == 3 + 6 and c1 == c + 3
    # blocks are added at slen 2, 66, ..., 386: 7 steps for each of the 5 query lengths (and slen 0 -> 1)
    assert steps == 5 * 8


@needs_hipcc
def test_order_is_a_stable_descending_permutation(batch_hits_check):
    m = re.search(r"order: (\d+) ties kept in order", batch_hits_check)
    assert m and int(m.group(1)) > 100, batch_hits_check


@needs_hipcc
def test_per_hit_groups(batch_hits_check):
    m = re.search(r"groups: (\d+) rounds split", batch_hits_check)
    assert m and int(m.group(1)) > 20, batch_hits_check


@pytest.mark.parametrize("flags", [["--queries", "/nonexistent/qs.fasta"],
                                   ["--queries", "/nonexistent/qs.fasta", "--hits", "5", "--query", "/nonexistent/q.fasta"],
                                   ["--queries", "/nonexistent/qs.fasta", "--hits", "5", "--pssm", "/nonexistent/p.txt"],
                                   ["--queries", "/nonexistent/qs.fasta", "--hits", "5", "--gpus", "2"],
                                   ["--queries", "/nonexistent/qs.fasta", "--topk", "5", "--gpus", "2"],
                                   ["--queries", "/nonexistent/qs.fasta", "--topk", "5000"],
                                   ["--queries", "/nonexistent/qs.fasta", "--hits", "0"],
                                   ["--queries", "/nonexistent/qs.fasta", "--hits", "5", "--topk", "5"],
                                   ["--queries", "/nonexistent/qs.fasta", "--hits", "5", "--make-db", "/nonexistent/o.swdb"]])
def test_cli_rejects_bad_queries_flags(flags):
    """Exit 1 with a message naming --queries, before any file is read (the
    files named here do not exist)."""
    out = subprocess.run([os.path.join(LIB, "main"), "--db", "/nonexistent/db.fasta"] + flags, capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 1 and "--queries" in out.stderr, (out.stdout, out.stderr)


def test_cli_usage_lists_queries():
    out = subprocess.run([os.path.join(LIB, "main"), "--help"], capture_output=True, text=True, timeout=60)
    assert "--queries" in out.stdout and "--hits" in out.stdout


def test_cli_names_an_unreadable_queries_file():
    out = subprocess.run([os.path.join(LIB, "main"), "--db", "/nonexistent/db.fasta", "--queries", "/nonexistent/qs.fasta",
                          "--hits", "5"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "--queries" in out.stderr and "/nonexistent/qs.fasta" in out.stderr


@pytest.fixture(scope="module")
def read_queries(tmp_path_factory):
    """The stand-alone reader: swsolver.cpp as the CLI builds it, linked with the library."""
    tmp = tmp_path_factory.mktemp("read_queries")
    exe = str(tmp / "read_queries_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall"] + INC +
                   [os.path.join(ROOT, "tests", "native", "read_queries_check.cpp"), os.path.join(CSRC, "swsolver.cpp"),
                    "-o", exe, "-L" + LIB, "-lswamd", "-lpthread", "-Wl,-rpath," + LIB], check=True, timeout=300)

    def run(text):
        path = tmp / "q.fasta"
        path.write_text(text)
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
        return r.returncode, r.stdout.split("\n")[:-1]
    return run


def test_read_queries_records(read_queries):
    """Three records with blank lines between and inside them, a header with
    spaces (the name is its first word), residues over several lines."""
    rc, out = read_queries("\n>sp|P1|ONE first protein  of three\nMKV\n\nLLA\n\n>two\nACDEFGHIK\n\n\n>three more words\nW\nY\n")
    assert rc == 0
    assert out == ["records 3", "sp|P1|ONE|6|MKVLLA", "two|9|ACDEFGHIK", "three|2|WY"]


def test_read_queries_empty_record_and_names(read_queries):
    """A record with no residues stays a record (an empty query); a bare '>'
    has an empty name; CR line ends and trailing blanks are dropped."""
    rc, out = read_queries(">a\r\nMK \r\n>empty\n>\nAA\n>  padded name\nC")
    assert rc == 0
    assert out == ["records 4", "a|2|MK", "empty|0|", "|2|AA", "padded|1|C"]


@pytest.mark.parametrize("text", ["", "MKVLLA\nACD\n", "\n\n", "MKV\n>late\nAC\n"])
def test_read_queries_rejects_a_file_without_a_header(read_queries, text):
    rc, out = read_queries(text)
    assert rc == 1 and out and out[0].startswith("error: ") and "q.fasta" in out[0], out
