"""Differential of two builds of lib/main on a machine without a GPU:

    python profiles/r13_cli_one_path/diff_cli.py OLD_MAIN NEW_MAIN

Runs both over every argument list of tests/golden/record_cli_flag_cases.py
(the 1,160 subsets, accepted ones included: without a GPU they end in the
library's own error), the same lists with a .swdb database path, and the
hand-written EXTRA lists (value forms, precedence around a --matrix file,
flags without a value).  Exit code, stdout and stderr must be identical, but
for the wall-time lines.  Prints one line per difference and a count."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
spec = importlib.util.spec_from_file_location("rec", os.path.join(ROOT, "tests", "golden", "record_cli_flag_cases.py"))
rec = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rec)

Q, DB = ["--query", "/nonexistent/q.fasta"], ["--db", "/nonexistent/db.fasta"]
EXTRA = [
    Q + DB + ["--matrix", "/nonexistent/m.txt", "--gap-open", "0"],  # the file's error goes first
    Q + DB + ["--matrix", "/nonexistent/m.txt", "--topk", "0"],
    Q + DB + ["--matrix", "BLOSUM62", "--gap-extend", "x"],
    Q + DB + ["--gap-open", "3", "--gap-extend", "1001"],
    Q + DB + ["--gap-open=0"], Q + DB + ["--topk=7"], Q + DB + ["--topk", "5000"], Q + DB + ["--topk", " 5"],
    Q + DB + ["--topk", "5x"], Q + DB + ["--gpus", "0"], Q + DB + ["--gpus", "x"], Q + DB + ["--gpus", "1"],
    Q + DB + ["--gpus", "2x", "--hits", "5"], Q + DB + ["--hits", "5", "--gpus", "1"],
    Q + DB + ["--hits", "4097"], Q + DB + ["--hits", ""], Q + DB + ["--hits=5", "--evalue=yes"],
    Q + DB + ["--hits", "5", "--evalue", "--rank", "evalue", "--max-evalue", "inf"],
    Q + DB + ["--hits", "5", "--evalue", "--rank", "evalue", "--max-evalue", "nan"],
    Q + DB + ["--hits", "5", "--evalue", "--rank", "evalue", "--max-evalue", "1e-3x"],
    Q + DB + ["--hits", "5", "--hits", "0"], Q + DB + ["--hits", "0", "--hits", "5"],
    Q + DB + ["--metrics-json"], Q + DB + ["--metrics-json=1", "--topk", "3"],
    ["--help=1"], ["positional"], Q + ["--db"], Q + DB + ["--frobnicate"], Q + DB + ["--evalue", "--frobnicate"],
    ["--frobnicate=1", "--help"], ["--help", "--frobnicate", "1"], ["--query"], ["--evalue"], ["--metrics-json"],
    ["--pssm", "/nonexistent/p.pssm", "--query", "/nonexistent/q.fasta", "--help"],
    ["--pssm", "/nonexistent/p.pssm"] + DB + ["--gpus", "2"], ["--pssm", "/nonexistent/p.pssm"] + DB + ["--gpus", "1"],
    ["--pssm", "/nonexistent/p.pssm"] + DB + ["--gap-open", "0"],
    ["--queries", "/nonexistent/qs.fasta"] + DB + ["--topk", "4097"],
    ["--queries", "/nonexistent/qs.fasta"] + DB + ["--hits", "5", "--gpus", "1"],
    ["--make-db", "/nonexistent/out.swdb"] + DB + ["--topk", "0", "--gpus", "0"],
    ["--make-db", "/nonexistent/out.swdb", "--db", "/nonexistent/db.swdb"],
]


def stable(text):
    return [ln for ln in text.split("\n") if not ln.startswith(("Time elapsed:", "Performance:", '{"query_len"'))]


def main():
    old, new = sys.argv[1], sys.argv[2]
    lists = rec.cases()
    lists += [[a.replace("db.fasta", "db.swdb") for a in args] for args in rec.cases() if "--db" in args]
    lists += EXTRA
    differ = 0
    for args in lists:
        a, b = rec.run(old, args), rec.run(new, args)
        if (a[0], stable(a[1]), a[2]) != (b[0], stable(b[1]), b[2]):
            differ += 1
            print("DIFFERS: %s\n  old: %r\n  new: %r" % (" ".join(args), a, b))
    print("%d argument lists, %d differ" % (len(lists), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
