"""Records the transcripts tests/test_gpu_cli_modes.py compares against.

    python tests/golden/cli_modes/record.py MAIN [OUTDIR]

MAIN is the `main` of the commit whose output is to be pinned (a build of it
kept apart from lib/); the cases, the command lines and the filtering are the
test's own.  A case whose FASTA and .swdb runs print the same is written once,
as NAME.txt; otherwise as NAME.fasta.txt and NAME.swdb.txt.  query.pssm, the
profile of the --pssm modes, is written when it is missing: 48 positions over
P01008's residues 31..78, seeded noise with a high score on the residue
itself.  Needs a GPU; stops at the first run that ends abnormally."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import test_gpu_cli_modes as T  # noqa: E402

LETTERS = "ARNDCQEGHILKMFPSTWYVBJZX*"


def write_pssm(path):
    with open(os.path.join(T.GOLDEN, "queries", "P01008.fasta")) as f:
        seq = "".join(f.read().split("\n")[1:])[30:78]
    rng = np.random.default_rng(20261021)
    with open(path, "w") as f:
        f.write("# position-specific scoring matrix, %d positions\n" % len(seq))
        f.write("      " + " ".join("%4s" % c for c in LETTERS) + "\n")
        for i, c in enumerate(seq):
            row = rng.integers(-4, 3, size=25)
            row[LETTERS.index(c)] = rng.integers(4, 9)
            row[23], row[24] = -1, -4
            f.write("%4d %s " % (i + 1, c) + " ".join("%4d" % int(x) for x in row) + "\n")


def main():
    exe = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else T.MODES_DIR
    os.makedirs(out, exist_ok=True)
    if not os.path.exists(T.PSSM[1]):
        write_pssm(T.PSSM[1])
    with tempfile.TemporaryDirectory() as tmp:
        dbs = {"fasta": os.path.join(T.GOLDEN, "subset111.fasta"),
               "swdb": T.make_swdb(exe, os.path.join(tmp, "subset111.swdb"))}
        for case in T.CASES:
            texts = {}
            for source in T.SOURCES:
                texts[source], _ = T.run_case(exe, dbs[source], *case)
                if not texts[source].startswith(("exit 0\n", "exit 1\n")):
                    sys.exit("%s %s: %s" % (T.case_name(*case), source, texts[source][-2000:]))
            name = T.case_name(*case)
            same = texts["fasta"] == texts["swdb"]
            for source in T.SOURCES[:1] if same else T.SOURCES:
                with open(os.path.join(out, name + (".txt" if same else ".%s.txt" % source)), "w") as f:
                    f.write(texts[source])
            print(name, "both sources agree" if same else "the sources differ", texts["fasta"].split("\n")[0], flush=True)


if __name__ == "__main__":
    main()
