"""The workspace layouts of the search and rollout drivers stay what they were before the four search drivers became one
(tests/search_layout_cases.py; the values in tests/golden/search_layouts.json were recorded on a build of that earlier
commit), and the single search is the one-member ensemble that records its attention maps.  No GPU: the queries launch
nothing."""
import pytest

import search_layout_cases as SL

CASES = SL.cases()


def test_the_table_is_the_recorded_one():
    assert sorted(SL.golden()) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_bytes_and_offsets_are_the_recorded_ones(case):
    fn, args = CASES[case]
    nbytes, off = fn(*args)
    want_bytes, want_off = SL.golden()[case]
    assert nbytes == want_bytes
    assert off == want_off


@pytest.mark.parametrize("options", [0, 1])
@pytest.mark.parametrize("K,T", SL.KT)
@pytest.mark.parametrize("name", sorted(SL.DIMS))
def test_single_is_the_one_member_ensemble(name, K, T, options):
    alpha_member = 0 if SL.DIMS[name][-1] else -1
    assert SL.single(name, K, T, options) == SL.ensemble((name,), K, T, alpha_member, options)
