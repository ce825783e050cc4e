"""The code-plane entry points against tests/golden/code_plane_refusals.json (tools/make_golden_refusals.py): status and full
message of every single violation and of every pair of two -- the texts byte for byte, and which of two broken rules is reported.
No GPU: every call is refused on the host, over addresses that are never dereferenced."""
import json
import os

import pytest

from codon_amd import _lib as L
from tests import code_plane_calls as calls

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "code_plane_refusals.json")
with open(GOLDEN) as _fh:
    DOC = json.load(_fh)


def test_the_golden_covers_every_entry_and_is_small():
    assert set(DOC["entries"]) == set(calls.ENTRIES) == set(calls.VIOLATIONS) and len(calls.ENTRIES) == 11
    assert DOC["provenance"]["abi_version"] == L.ABI_VERSION and len(DOC["provenance"]["commit"]) == 40
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert all(st != 0 for st, _ in DOC["strings"])                     # nothing recorded was accepted: nothing replayed may launch
    for entry, rec in DOC["entries"].items():
        n = len(rec["violations"])
        assert n >= len(calls.VIOLATIONS[entry]) and len(rec["single"]) == n and len(rec["pairs"]) == n * (n - 1) // 2, entry


@pytest.mark.parametrize("entry", sorted(calls.ENTRIES))
def test_refusals_replay_byte_for_byte(entry):
    lib = L.load()
    rec = DOC["entries"][entry]
    want = rec["single"] + rec["pairs"]
    cases = calls.cases(rec["violations"])
    assert len(cases) == len(want)
    for kw, k in zip(cases, want):
        st, msg = DOC["strings"][k]
        assert calls.call(lib, entry, kw) == (st, msg), (entry, kw)
