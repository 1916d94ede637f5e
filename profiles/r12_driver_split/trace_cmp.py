"""Compare two rocprofv3 --hip-runtime-trace runs of trace_calls.py (argv: the
two output directories): the HIP calls, in order of their start, each with its
thread (threads numbered by first appearance)."""
import csv
import glob
import sys
from collections import Counter


def load(d):
    files = glob.glob(d + "/**/*hip_api_trace.csv", recursive=True)
    assert len(files) == 1, (d, files)
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    tid, seq = {}, []
    for r in rows:
        seq.append((tid.setdefault(r["Thread_Id"], len(tid)), r["Function"]))
    return seq


def library_calls(seq):
    """From the handle's first stream on (what precedes is the interpreter's
    and the runtime's start-up)."""
    return seq[next(i for i, (_, f) in enumerate(seq) if f == "hipStreamCreateWithFlags"):]


a, b = load(sys.argv[1]), load(sys.argv[2])
print("calls", len(a), len(b), "threads", len({t for t, _ in a}), len({t for t, _ in b}))
ta, tb = library_calls(a), library_calls(b)
print("from the handle's first stream on:", len(ta), len(tb))
for i, (x, y) in enumerate(zip(ta, tb)):
    if x != y:
        print("first difference at", i, x, y, ta[max(0, i - 5):i + 5], tb[max(0, i - 5):i + 5])
        break
print(Counter(f for _, f in ta).most_common(40))
print("SAME" if ta == tb else "DIFFERENT")
sys.exit(0 if ta == tb else 1)
