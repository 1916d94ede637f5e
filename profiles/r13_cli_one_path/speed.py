"""main --metrics-json, the parent's build and this tree's alternating, five runs each, on the
570,000-record synthetic FASTA of scripts/dropin_scale.py (the largest the tree generates offline):

    python profiles/r13_cli_one_path/speed.py PARENT_MAIN [OUT.json]

PARENT_MAIN is the parent commit's lib/main beside its own libswamd.so.  Needs a GPU."""
import json, os, subprocess, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "scripts"))
import _swpkg, dropin_scale
sw = _swpkg.load()
mains = {"parent": os.path.abspath(sys.argv[1]),
         "new": os.path.join(REPO, "ece1782-smith-waterman-cuda_amd", "lib", "main")}
query = os.path.join(REPO, "tests", "golden", "queries", "P07327.fasta")
out = {"records": 570000, "runs": {"parent": [], "new": []}}
with tempfile.TemporaryDirectory() as tmp:
    fasta = os.path.join(tmp, "synth570000.fasta")
    t = time.time()
    res, offs = sw.synth.database(570000, shard=0)
    dropin_scale.write_fasta(fasta, res, offs)
    out["fasta_bytes"] = os.path.getsize(fasta); out["fasta_write_s"] = round(time.time() - t, 1)
    print("fasta written", out["fasta_bytes"], out["fasta_write_s"], flush=True)
    digest = {}
    for i in range(5):
        for name in ("parent", "new"):
            r = subprocess.run([mains[name], "--query", query, "--db", fasta, "--metrics-json"], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit("%s run %d: exit %d: %s" % (name, i, r.returncode, r.stderr[-1000:]))
            lines = r.stdout.split("\n")
            m = json.loads([ln for ln in lines if ln.startswith('{"query_len"')][0])
            out["runs"][name].append(m)
            body = "\n".join(ln for ln in lines if not ln.startswith(("Time elapsed:", "Performance:", '{"query_len"')))
            digest.setdefault(name, set()).add(hash(body))
            print(name, i, m["solve_s"], m["wall_s"], m["parse_s"], m["flatten_s"], m["upload_s"], m["scan_s"], flush=True)
    out["outputs_identical"] = len(digest["parent"] | digest["new"]) == 1
for name in ("parent", "new"):
    s = sorted(m["solve_s"] for m in out["runs"][name])
    out[name + "_solve_s"] = {"min": s[0], "median": s[2], "max": s[-1]}
p, n = out["parent_solve_s"], out["new_solve_s"]
out["new_median_within_parent_spread"] = p["min"] <= n["median"] <= p["max"]
print(json.dumps({k: v for k, v in out.items() if k != "runs"}))
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "speed.json", "w"), indent=1)
