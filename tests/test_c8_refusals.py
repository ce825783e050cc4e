"""Every refusal of the entries that take a dtype or a 16-bit slice is made with the return code and under the entry-point name
(the text before the first ':') of the commit before the 16-bit host rules were stated once:
tests/golden/c8_refusals.json, recorded with tests/c8_refusals.py.  The cases carry fake pointers, so the module runs only where
there is no GPU: a case that wrongly stopped refusing must never reach a launch."""
import json
import os

import pytest
import torch

from tests import c8_refusals as R

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: CPU machines only")

CASES = R.cases()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "c8_refusals.json")) as f:
        return json.load(f)


def test_same_cases_as_the_golden(golden):
    assert sorted(golden) == sorted(R.case_id(n, c) for n, c, _ in CASES)
    assert all(code in (-1, -2) for code, _ in golden.values())          # BAD_ARG / UNSUPPORTED: refused, never launched


def test_every_refusal_is_the_parent_commits(golden):
    wrong = {}
    for name, case, over in CASES:
        want = golden[R.case_id(name, case)]
        assert want[0] in (-1, -2), (name, case, want)                   # a recorded refusal: nothing here may reach a launch
        got = list(R.call(name, over))
        if got != want:
            wrong[R.case_id(name, case)] = (got, want)
    assert not wrong, f"{len(wrong)} of {len(CASES)} refusals changed (got, want): {dict(list(wrong.items())[:8])}"
