"""Wall time of sw_db_create on C2's 570,000 subjects: dbtime.py ROOT -> one JSON line."""
import json, os, sys, time
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import _swpkg
sw = _swpkg.load()
res, offs = sw.synth.database(570000, shard=0)
h = sw.Handle(0, env_opts=False)
ts = []
for i in range(4):
    t0 = time.perf_counter()
    db = sw.Database(h, res, offs)
    t = time.perf_counter() - t0
    st = db.stats()
    db.close()
    ts.append(t)
h.close()
timed = sorted(ts[1:])
print(json.dumps({"root": root, "build_id": sw.capi.build_id(), "first_s": round(ts[0], 4),
                  "timed_s": [round(x, 4) for x in ts[1:]], "median_s": round(timed[1], 4),
                  "n_blocks": st.get("n_blocks") if isinstance(st, dict) else str(st)}))
