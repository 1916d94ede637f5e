"""Records tests/golden/cli_flag_cases.json: what `main` answers to argument
lists it can decide without the library.

    python tests/golden/record_cli_flag_cases.py OBJDIR [OUT.json]

OBJDIR holds main.host.o and swsolver.host.o of the commit to record (the
fixture in the tree comes from the last commit whose main.cpp checked its
flags inline).  The two objects are linked against a stub libswamd.so made
here, in which every function of include/sw_amd.h prints a marker and exits
with STUB_EXIT: a case that ends so has touched the library and is left out.
The cases are every subset of up to three of FLAGS, in FLAGS' order, over
paths that do not exist.  The usage text, which most cases print, is stored
once: a case's "stdout" is "" or "@usage"."""
import itertools
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
STUB_EXIT = 99
FLAGS = [["--query", "/nonexistent/q.fasta"], ["--queries", "/nonexistent/qs.fasta"], ["--pssm", "/nonexistent/p.pssm"],
         ["--db", "/nonexistent/db.fasta"], ["--hits", "5"], ["--hits", "0"], ["--topk", "5"], ["--topk", "0"],
         ["--evalue"], ["--rank", "evalue"], ["--rank", "score"], ["--max-evalue", "1"], ["--max-evalue", "0"],
         ["--gpus", "2"], ["--make-db", "/nonexistent/out.swdb"], ["--matrix", "blosum62"], ["--gap-open", "0"],
         ["--help"], ["--frobnicate", "1"]]


def cases():
    """Every argument list: the subsets of up to three flags."""
    return [sum(c, []) for r in range(4) for c in itertools.combinations(FLAGS, r)]


def run(exe, args):
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    return out.returncode, out.stdout, out.stderr


def stub_main(objdir, tmp):
    """The commit's main over a library that only says it was called."""
    with open(os.path.join(ROOT, "include", "sw_amd.h")) as f:
        names = re.findall(r"^SW_API\s+[\w\s\*]+?\b(sw_\w+)\s*\(", f.read(), re.M)
    assert "sw_create" in names and "sw_encode" in names and len(names) > 70, names
    src = os.path.join(tmp, "stub.c")
    with open(src, "w") as f:
        f.write("#include <stdio.h>\n#include <unistd.h>\n")
        f.write("static void touched(const char* name) { fprintf(stderr, \"library touched: %%s\\n\", name);"
                " fflush(stderr); _exit(%d); }\n" % STUB_EXIT)
        for name in names:
            f.write("void %s(void) { touched(\"%s\"); }\n" % (name, name))
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", os.path.join(tmp, "libswamd.so"), src], check=True)
    exe = os.path.join(tmp, "main")
    subprocess.run(["g++", "-o", exe, os.path.join(objdir, "main.host.o"), os.path.join(objdir, "swsolver.host.o"),
                    "-L" + tmp, "-lswamd", "-lpthread", "-Wl,-rpath," + tmp], check=True)
    return exe


def main():
    objdir = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "cli_flag_cases.json")
    with tempfile.TemporaryDirectory() as tmp:
        exe = stub_main(objdir, tmp)
        usage = run(exe, ["--help"])[1]
        kept, touched = [], 0
        for args in cases():
            code, stdout, stderr = run(exe, args)
            if code == STUB_EXIT:
                touched += 1
                continue
            assert code in (0, 1) and stdout in ("", usage), (args, code, stdout)
            kept.append({"args": args, "code": code, "stdout": "@usage" if stdout else "", "stderr": stderr})
    with open(out, "w") as f:
        f.write('{"usage": %s,\n "cases": [\n' % json.dumps(usage))
        f.write(",\n".join("  " + json.dumps(c) for c in kept))
        f.write("\n ]}\n")
    print("%d cases kept, %d touched the library" % (len(kept), touched))


if __name__ == "__main__":
    main()
