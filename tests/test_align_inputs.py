"""CPU: the tie set of tests/align_support.py can tell the traceback's rules
apart.  The Python restatement of the rules equals the oracle on every pair
and scoring of the set, and each wrong rule (align_support.VARIANTS) differs
from the oracle on at least three of them: a condition on the inputs, so that
the GPU comparison on the same set (tests/test_gpu_align_rules.py) cannot pass
with a tie rule wrong."""
import pytest

from align_support import AFFINE_ONLY, SCORINGS, VARIANTS, align_py, is_affine, scoring, tie_cases
from conftest import path_score


@pytest.fixture(scope="module")
def cases(oracle):
    """[(scoring name, query, subject, matrix, go, ge, the oracle's alignment)]"""
    out = []
    for name in SCORINGS:
        mat, go, ge = scoring(name)
        for _, _, q, s in tie_cases(name):
            out.append((name, q.tolist(), s.tolist(), mat, go, ge, oracle.align(q, s, mat, go, ge)))
    return out


def test_set_shape():
    lin = [n for n in SCORINGS if not is_affine(n)]
    aff = [n for n in SCORINGS if is_affine(n)]
    for names in (lin, aff):  # an I D pair beats a mismatch under each gap model
        assert any(2 * SCORINGS[n][3] < -SCORINGS[n][2] for n in names)
    for name in SCORINGS:
        assert SCORINGS[name][0] in (2, 3)
        for _, _, q, s in tie_cases(name):
            assert 1 <= len(q) <= 40 and 1 <= len(s) <= 40 and max(q.max(), s.max()) < SCORINGS[name][0]


def test_restatement_equals_the_oracle(cases):
    gapped = 0
    for name, q, s, mat, go, ge, want in cases:
        got = align_py(q, s, mat, go, ge)
        assert got == want, (name, q, s, got, want)
        if want["score"] > 0:
            assert path_score(q, s, mat, go, ge, want) == want["score"]
        gapped += "I" in want["ops"] or "D" in want["ops"]
    assert 4 * gapped >= len(cases), "a quarter of the paths hold a gap"


@pytest.mark.parametrize("variant", VARIANTS)
def test_each_wrong_rule_shows(cases, variant):
    """At least 3 (pair, scoring) cases on which the wrong rule's alignment is
    not the oracle's, under each gap model the rule applies to; the wrong
    alignment is still optimal (its path scores the oracle's score)."""
    differ = {False: 0, True: 0}
    for name, q, s, mat, go, ge, want in cases:
        if variant in AFFINE_ONLY and not is_affine(name):
            continue
        got = align_py(q, s, mat, go, ge, variant=variant)
        assert got["score"] == want["score"]
        if got["score"] > 0:
            assert path_score(q, s, mat, go, ge, got) == got["score"]
        differ[is_affine(name)] += got != want
    print("%s: differs on %d linear and %d affine cases" % (variant, differ[False], differ[True]))
    assert differ[True] >= 3, (variant, differ)
    if variant not in AFFINE_ONLY:
        assert differ[False] >= 3, (variant, differ)


def test_oracle_short_buffer_holds_the_paths_first_ops(oracle, cases):
    """swo_align_linear / swo_align_affine with ops_cap below the path length:
    the begin of the path, from (q_begin, s_begin), and the full ops_len."""
    seen = 0
    for name, q, s, mat, go, ge, want in cases[::7]:
        full = want["ops"]
        for cap in sorted({0, 1, 7, max(len(full) - 1, 0), len(full), len(full) + 1}):
            got = oracle.align(q, s, mat, go, ge, ops_cap=cap)
            assert got.pop("ops_len") == len(full)
            assert got == dict(want, ops=full[:cap]), (name, q, s, cap, got, want)
            seen += cap < len(full) and full[:cap] != full[len(full) - cap:]
    assert seen > 100, "buffers whose prefix is not the path's suffix"
