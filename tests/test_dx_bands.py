"""The split input gradient's row-band schedule (native_ops._dx_bands): the
order of its groups is what "dX is bitwise the same in every mode" rests on."""
import pytest

from pytorch_end2end_speech_recognition_amd.native_ops import _dx_bands

_CASES = [(T, two) for T in range(64, 301) for two in (False, True) if T >= 128 or not two]


@pytest.mark.parametrize('two', [False, True])
def test_every_length_is_covered_once_in_the_fixed_order(two):
    """Every T in 64..300 (two chunks where the caller uses them, T >= 128):
    the ranges of all groups are disjoint and cover [0, T) exactly; the middle
    band first, with two chunks the second pair next, the two outer ranges
    last.  (T = 64, 67, 128, 130: where T//4 or T//8 would be off by one.)"""
    for T, _ in (c for c in _CASES if c[1] == two):
        groups = _dx_bands(T, two)
        assert len(groups) == (3 if two else 2), (T, groups)
        ranges = sorted(r for g in groups for r in g)
        assert all(ta < tb for ta, tb in ranges), (T, ranges)
        assert ranges[0][0] == 0 and ranges[-1][1] == T, (T, ranges)
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), (T, ranges)
        assert groups[0] == [(T // 4, T - T // 4)], (T, groups)
        outer = T // 4
        if two:
            assert groups[1] == [(T // 8, T // 4), (T - T // 4, T - T // 8)], (T, groups)
            outer = T // 8
        assert groups[-1] == [(0, outer), (T - outer, T)], (T, groups)


def test_off_by_one_lengths():
    assert _dx_bands(64, False) == [[(16, 48)], [(0, 16), (48, 64)]]
    assert _dx_bands(67, False) == [[(16, 51)], [(0, 16), (51, 67)]]
    assert _dx_bands(128, True) == [[(32, 96)], [(16, 32), (96, 112)], [(0, 16), (112, 128)]]
    assert _dx_bands(130, True) == [[(32, 98)], [(16, 32), (98, 114)], [(0, 16), (114, 130)]]
