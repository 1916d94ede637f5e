"""GPU: every mode of `lib/main`, byte for byte against transcripts recorded
from the commit before the CLI's two front ends (FASTA through the drop-in
functions, .swdb through the raw C ABI) became one search path
(tests/golden/cli_modes/, recorded by its record.py).

Each case runs main on the 111-record subset as FASTA and as the .swdb file
`--make-db` writes from it.  stdout is compared without the lines that carry
wall time (`Time elapsed:`, `Performance:`, the --metrics-json line), stderr
whole.  A transcript `NAME.txt` holds what both sources printed when they were
recorded, so it also pins that they agree; where they did not, `NAME.fasta.txt`
and `NAME.swdb.txt` hold each one's."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "lib")
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODES_DIR = os.path.join(GOLDEN, "cli_modes")

QUERY = ["--query", os.path.join(GOLDEN, "queries", "P01008.fasta")]
QUERIES = ["--queries", os.path.join(GOLDEN, "calib_queries.fasta")]
PSSM = ["--pssm", os.path.join(MODES_DIR, "query.pssm")]
MODES = {
    "scan": QUERY,
    "topk10": QUERY + ["--topk", "10"],
    "topk5000": QUERY + ["--topk", "5000"],  # above the device top-K's 4096: ranked on the host
    "hits5": QUERY + ["--hits", "5"],
    "hits5_evalue": QUERY + ["--hits", "5", "--evalue"],
    "hits5_ranked": QUERY + ["--hits", "5", "--evalue", "--rank", "evalue", "--max-evalue", "10"],
    "queries_topk3": QUERIES + ["--topk", "3"],
    "queries_hits3": QUERIES + ["--hits", "3"],
    "queries_hits3_evalue": QUERIES + ["--hits", "3", "--evalue"],
    "queries_hits3_ranked": QUERIES + ["--hits", "3", "--evalue", "--rank", "evalue"],
    "pssm": PSSM,
    "pssm_topk10": PSSM + ["--topk", "10"],
}
# the reference's scoring, and a set one (--matrix cannot be combined with --pssm: its gaps alone)
SCORINGS = {
    "ref": lambda mode: [],
    "set": lambda mode: (["--gap-open", "12", "--gap-extend", "1"] if mode.startswith("pssm") else
                         ["--matrix", "blosum62", "--gap-open", "12", "--gap-extend", "1"]),
}
# (mode, scoring, gpus): --gpus 2 over one device listed twice; a .swdb database ignores it
CASES = [(m, s, 1) for m in MODES for s in SCORINGS] + [(m, s, 2) for m in ("scan", "topk10") for s in SCORINGS]
SOURCES = ("fasta", "swdb")
METRICS_KEYS = ["query_len", "subjects", "padded_residues", "wall_s", "parse_s", "solve_s", "flatten_s", "init_s",
                "upload_s", "scan_s", "gpus"]


def case_name(mode, scoring, gpus):
    return "%s.%s%s" % (mode, scoring, ".gpus2" if gpus == 2 else "")


def run_case(main, db, mode, scoring, gpus):
    """One run of `main`: (transcript, the --metrics-json line or None)."""
    args = [main, "--db", db] + MODES[mode] + SCORINGS[scoring](mode) + ["--metrics-json"]
    env = dict(os.environ)
    for name in ("SW_GPUS", "SW_DEVICES", "SW_DEVICE", "SW_CHAR_COMPAT"):
        env.pop(name, None)
    if gpus == 2:
        args += ["--gpus", "2"]
        env["SW_DEVICES"] = "0,0"
    out = subprocess.run(args, capture_output=True, text=True, timeout=120, env=env)
    lines = out.stdout.split("\n")
    metrics = [ln for ln in lines if ln.startswith('{"query_len"')]
    kept = [ln for ln in lines if not ln.startswith(("Time elapsed:", "Performance:", '{"query_len"'))]
    text = "exit %d\n--- stdout ---\n%s\n--- stderr ---\n%s" % (out.returncode, "\n".join(kept), out.stderr)
    return text, (metrics[0] if metrics else None)


def make_swdb(main, path):
    mk = subprocess.run([main, "--make-db", path, "--db", os.path.join(GOLDEN, "subset111.fasta")],
                        capture_output=True, text=True, timeout=120)
    assert mk.returncode == 0, mk.stdout + mk.stderr
    return path


@pytest.fixture(scope="module")
def databases(tmp_path_factory):
    main = os.path.join(LIB, "main")
    return {"fasta": os.path.join(GOLDEN, "subset111.fasta"),
            "swdb": make_swdb(main, str(tmp_path_factory.mktemp("cli_modes") / "subset111.swdb"))}


def recorded(name, source):
    both = os.path.join(MODES_DIR, name + ".txt")
    path = both if os.path.exists(both) else os.path.join(MODES_DIR, "%s.%s.txt" % (name, source))
    with open(path) as f:
        return f.read()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,scoring,gpus", CASES, ids=[case_name(*c) for c in CASES])
def test_mode_prints_what_it_printed_before(databases, mode, scoring, gpus):
    main = os.path.join(LIB, "main")
    for source in SOURCES:
        text, metrics = run_case(main, databases[source], mode, scoring, gpus)
        assert text == recorded(case_name(mode, scoring, gpus), source), (source, text[-3000:])
        assert metrics is not None and list(json.loads(metrics).keys()) == METRICS_KEYS, (source, metrics)
