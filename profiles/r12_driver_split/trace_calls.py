"""One process, the calls whose HIP sequence is compared between the trees
(run under rocprofv3 --hip-runtime-trace).  argv[1]: the tree's root."""
import hashlib
import os
import sys

import numpy as np

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import _swpkg  # noqa: E402

sw = _swpkg.load()
assert os.path.dirname(os.path.dirname(sw.capi.LIB_PATH)).startswith(os.path.join(root, "ece1782")), sw.capi.LIB_PATH
h = sw.Handle(0, env_opts=False)
r, o = sw.synth.database(3000, shard=5)
db = sw.Database(h, r, o)
m = sw.capi.builtin_matrix(1)
q1, q2 = sw.synth.query(300, shard=1), sw.synth.query(650, shard=2)
empty = np.zeros(0, np.uint8)
out = hashlib.sha256()


def add(x):
    out.update(repr(x).encode() if not isinstance(x, np.ndarray) else x.tobytes())


add(db.scan(q1, m, 11, 1))
add(db.scan_batch([q1, empty, q2], m, 11, 1))
rows, cal = db.scan_hits_sig(q1, 20, m, 11, 1)
add(rows), add(cal.as_dict())
rows, cals = db.scan_batch_hits_sig([q1, q2], 20, m, 11, 1)
add(rows), add([c.as_dict() for c in cals])
add(db.align(q1, [3, 77, 500, 1234, 2999], m, 11, 1))
p = sw.Pssm(h, np.random.default_rng(3).integers(-4, 9, size=(120, 25)).astype(np.int8))
keys, cal = db.scan_pssm_topk_calib(p, 15, 11, 1)
add(keys), add(cal.as_dict())
db.set_long_threshold(600)
add(db.scan(q2, m, 11, 1))
add(db.stats())
p.close()
db.close()
h.close()
print("build", sw.capi.build_id(), "results", out.hexdigest())
