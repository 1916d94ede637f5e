"""GPU: a plain bench.py run (no --full) on a small database: the result
line's contract, --steps as the number of timed steps, none of the legs that
--full adds, and --dump-outputs holding the last timed step's scores and
top-K, equal to the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, read_query

pytestmark = pytest.mark.gpu

N, K = 3000, 20  # more than one block of subjects, a few of them past the long threshold


def test_plain_run_line_and_dump(tmp_path, sw, oracle):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3",
                          "--warmup", "1", "--db-seqs", str(N), "--topk", str(K), "--long-threshold", "600",
                          "--dump-outputs", str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=240, cwd=REPO)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, "bench prints ONE JSON line"
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "GCUPS" and d["higher_is_better"] is True and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["cells_per_step"] / (d["ms_per_step"] * 1e-3) / 1e9) <= 0.01 * d["value"]
    assert "3 steps in" in out.stderr
    for k in ("sustained", "cold_warm", "reference_scoring", "parity", "cpu_baseline"):
        assert k not in d, k
    res, offs = sw.synth.database(N, shard=0)
    want = oracle.scan(sw.encode(read_query("P07327")), res, offs, mat=sw.capi.builtin_matrix(1), gap_open=12,
                       gap_extend=1, nthreads=4)
    got = np.load(str(tmp_path / "out" / "scores.npy"))
    assert got.dtype == np.float32 and got.shape == (1, N) and np.array_equal(got[0], want)
    ids = np.load(str(tmp_path / "out" / "topk_ids.npy"))
    sc = np.load(str(tmp_path / "out" / "topk_scores.npy"))
    keys = sw.dist.local_topk(want, np.arange(N, dtype=np.int32), K)
    want_ids, want_sc = sw.capi.decode_keys(keys)
    assert ids.dtype == sc.dtype == np.float64
    assert np.array_equal(ids[0], want_ids) and np.array_equal(sc[0], want_sc)
    assert d["top_hit"] == {"id": int(want_ids[0]), "score": int(want_sc[0])}
