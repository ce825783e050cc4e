"""The fp32 forward convs and the weight-gradient kernels return the bits they returned before their host code was moved
onto one tiling rule, one parameter fill per family and one internal header.  tests/golden/conv_bits.json
was recorded with tests/conv_bits.py on the commit before that change, on an MI355X, twice with equal results; every digest
must match -- the kernels use no floating-point atomics, so there is nothing to exclude.  Each group asserts the tiling
(codon_conv_tiling_f32) or the band plan (tests.bounds.wgrad_bands) its shape is there for before it runs anything."""
import json
import os

import pytest

from tests import conv_bits as CB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "conv_bits.json")) as f:
        return json.load(f)


def test_same_groups_as_the_golden(golden):
    assert sorted(golden) == sorted(CB.group_id(k, a) for k, a in CB.GROUPS)


@pytest.mark.parametrize("kind,args", CB.GROUPS, ids=[CB.group_id(k, a) for k, a in CB.GROUPS])
def test_bits_are_the_parent_commits(golden, kind, args):
    want = golden[CB.group_id(kind, args)]
    got = CB.group_digests(kind, args)
    assert sorted(got) == sorted(want)
    wrong = [case for case in sorted(want) if got[case] != want[case]]
    assert not wrong, f"{len(wrong)} of {len(want)} digests differ: {wrong[:8]}"
