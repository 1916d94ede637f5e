"""CPU: tests/native/pssm_oracle.cpp (the scalar PSSM restatement the GPU PSSM
tests compare against) pinned to the pinned oracle: for a table derived from
a sequence and a matrix (rows[i] = M[q[i]]) its scores and its alignments are
oracle/sw_oracle.c's, under a linear gap, an affine one, and an asymmetric
matrix (a transposed index would show).  Bit-exact, no tolerance."""
import numpy as np
import pytest

from pssm_support import PssmOracle, derived


@pytest.fixture(scope="module")
def pso(tmp_path_factory):
    return PssmOracle(tmp_path_factory.mktemp("pssm_oracle"))


def scorings(oracle):
    rng = np.random.default_rng(531)
    asym = rng.integers(-9, 10, size=(25, 25))
    np.fill_diagonal(asym, rng.integers(4, 13, size=25))
    asym = np.ascontiguousarray(asym, dtype=np.int8)
    assert (asym != asym.T).any()
    return {"b50-linear-2": (oracle.matrix(0), 2, 2), "b62-11-1": (oracle.matrix(1), 11, 1),
            "asym-13-3": (asym, 13, 3)}


@pytest.mark.parametrize("qlen", [40, 375])
@pytest.mark.parametrize("name", ["b50-linear-2", "b62-11-1", "asym-13-3"])
def test_derived_table_equals_the_oracle(sw, oracle, pso, name, qlen):
    mat, go, ge = scorings(oracle)[name]
    res, offs = sw.synth.database(200)
    q = sw.synth.query(qlen, shard=qlen)
    rows = derived(q, mat)
    assert rows.shape == (qlen, 25) and np.array_equal(rows[3], mat[q[3]])
    want = oracle.scan(q, res, offs, mat=mat, gap_open=go, gap_extend=ge)
    got = pso.scan(rows, res, offs, go, ge)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert want.max() > 0
    gapped = 0
    for k in range(200):
        s = res[offs[k]:offs[k + 1]]
        al = pso.align(rows, s, go, ge)
        assert al == oracle.align(q, s, mat, go, ge), k
        assert al["score"] == want[k]
        gapped += "I" in al["ops"] or "D" in al["ops"]
    assert gapped, "some alignment holds a gap"


def test_empty_inputs(pso):
    rows = np.zeros((0, 25), dtype=np.int8)
    assert pso.scan(rows, np.array([1, 2, 3], np.uint8), [0, 3]).tolist() == [0]
    z = {"score": 0, "q_end": 0, "s_end": 0, "q_begin": 0, "s_begin": 0, "ops": ""}
    assert pso.align(rows, np.array([1], np.uint8)) == z
    assert pso.align(np.ones((3, 25), np.int8), np.zeros(0, np.uint8)) == z
