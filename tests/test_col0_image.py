"""The column-0 image of the affine fp16 inter scan (csrc/sw_inter_x2.hip
X2Lds, stage_x2s, x2s_pass), on the CPU.

The high strip's profile image has a copy `hi0 = hi - 8 ge (2^16 + 1)` (mod
2^32) that column 0 of every 8-column sub-group reads, so that the diagonal sum
H + lo + hi0 of the H that was NOT rebased is, bit for bit, the sum H' + lo +
hi of the rebased H' = H - 8 ge in both halves.  The constant is the host's
swplan::cell_range diff[1], obtained here as tests/test_cell_range.py obtains
it (tests/native/cell_range_check.cpp, linked from sw_plan.cpp alone).

Checked for the five schemes of that test, every pair of profile entries min S
.. max S of the two strips, a row group's first row (whose entries carry - 16
ge as well) and the other rows, and H halves from the offset Z (the lowest
floor, which every stored H reaches) to the highest pattern whose sum stays at
or below cell_range's top:
  * the two dword sums are equal mod 2^32;
  * each 16-bit half of the sum is the integer H_half - 8 ge + S + 2 ge (+ the
    first row's - 16 ge) of its own strip, inside [lowest, top]: nothing
    crossed bit 16."""
import numpy as np
import pytest

from test_cell_range import SCHEMES, ranges  # noqa: F401  (the module-scoped fixture)

M32 = 2 ** 32
ROW_GROUP = 16


@pytest.mark.parametrize("name", list(SCHEMES))
def test_host_constant(ranges, name):  # noqa: F811
    ge = SCHEMES[name][3]
    reb = ranges[name]["diff"][1]
    assert reb >> 16 == reb & 0xffff == 8 * ge, hex(reb)
    assert reb == 8 * ge * 0x00010001


@pytest.mark.parametrize("first_row", [False, True], ids=["row", "group-first-row"])
@pytest.mark.parametrize("name", list(SCHEMES))
def test_column0_sum(ranges, name, first_row):  # noqa: F811
    mn, mx, go, ge = SCHEMES[name]
    c = ranges[name]
    reb = c["diff"][1]
    # stage_x2s: lo = the low strip's S + bias sign-extended to 32 bits, hi =
    # the high strip's (S + bias) << 16, hi0 = hi - reb; bias = 2 ge, a row
    # group's first row 16 ge less
    b = 2 * ge - (ROW_GROUP * ge if first_row else 0)
    s = np.arange(mn, mx + 1, dtype=np.int64)
    lo = ((s + b) % M32)[:, None, None, None]
    hi = (((s + b) << 16) % M32)[None, :, None, None]
    hi0 = (hi - reb) % M32
    top_h = c["top"] - mx - 2 * ge
    halves = np.array(sorted({c["z"], c["z"] + 1, c["z"] + 7 * ge, c["z"] + 22 * ge, c["guard"], top_h - 1, top_h}),
                      dtype=np.int64)
    hl, hh = halves[None, None, :, None], halves[None, None, None, :]
    H = (hh << 16) | hl
    new = (hi0 + lo + H) % M32
    old = (hi + lo + (H - reb) % M32) % M32
    assert new.shape == (len(s), len(s), len(halves), len(halves))
    assert np.array_equal(new, old), name
    want_l = hl - 8 * ge + s[:, None, None, None] + b
    want_h = hh - 8 * ge + s[None, :, None, None] + b
    for w in (want_l, want_h):
        assert c["lowest"] <= w.min() and w.max() <= c["top"], (name, int(w.min()), int(w.max()), c)
    assert np.array_equal(new & 0xffff, np.broadcast_to(want_l, new.shape)), name
    assert np.array_equal(new >> 16, np.broadcast_to(want_h, new.shape)), name
