"""Every kernel of the 16-bit channel-blocked path returns the bits it returned before its host code was moved onto one element
dispatch, one preamble, one tile-grid function and one shape table.  tests/golden/c8_bits.json was recorded with
tests/c8_bits.py on the commit before that change, on an MI355X, twice with equal results; every digest must match -- none of
these kernels uses a floating-point atomic, so no group is excluded.  The groups that rest on a launch form (staged / resident
conv3x3, the head's band height, the statistics tile) assert it before they run anything."""
import json
import os

import pytest

from tests import c8_bits as CB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "c8_bits.json")) as f:
        return json.load(f)


def test_same_groups_as_the_golden_and_none_excluded(golden):
    assert CB.EXCLUDED == []
    assert sorted(golden) == sorted(CB.group_id(k, dn) for k, dn in CB.GROUPS)


@pytest.mark.parametrize("kind,dn", CB.GROUPS, ids=[CB.group_id(k, dn) for k, dn in CB.GROUPS])
def test_bits_are_the_parent_commits(golden, kind, dn):
    want = golden[CB.group_id(kind, dn)]
    got = CB.group_digests(kind, dn)
    assert sorted(got) == sorted(want)
    wrong = [case for case in sorted(want) if got[case] != want[case]]
    assert not wrong, f"{len(wrong)} of {len(want)} digests differ: {wrong[:8]}"
