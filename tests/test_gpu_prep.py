"""The low-resolution depth preparation issues the launches it always did: the ordered call log of
tests/abi_log_prep.py -- infer.run_loop in both loops, train.TrainSet, train.synthesize and train.validate under every combination
of hole filling, guided filling and range normalisation, 8-bit and 16-bit -- equals, scenario by scenario and argument by argument,
the log recorded on the commit before the preparation got one record (tests/golden/abi_log_prep.json), and so do the SHA-256 of
the pool after TrainSet and of the depth input the network was handed."""
import json
import os

import pytest

from tests import abi_log_prep as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_call_log_and_bytes_equal_the_recorded_ones(tmp_path):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_log_prep.json")))
    got = json.loads(json.dumps(A.record(str(tmp_path))))           # tuples and lists compare as the JSON holds them
    assert set(got) == set(want) == set(A.FORMATS)
    for fmt in A.FORMATS:
        assert set(got[fmt]) == set(want[fmt]) == set(A.COMBOS) | {"degrade_fill"}
        for combo, scenarios in want[fmt].items():
            if combo == "degrade_fill":
                assert got[fmt][combo] == scenarios, (fmt, combo)
                continue
            assert set(got[fmt][combo]) == set(scenarios)
            for name, calls in scenarios.items():
                assert got[fmt][combo][name] == calls, (fmt, combo, name)
            assert scenarios["serial_input_sha256"] == scenarios["pipelined_input_sha256"]
    # the recorded logs are not vacuous: every kernel of the preparation is in them, and the options reach the bytes
    full = want["u16"]["fill_guided_normalize"]
    assert [c[0] for c in full["serial"][:6]] == ["codon_fill_holes_guided", "codon_code_range", "codon_stretch_codes",
                                                  "codon_lr_codes_to_input", "codon_postprocess_u16_dt", "codon_unstretch_codes"]
    assert full["pipelined"] == {"s0": full["serial"]}
    assert [c[0] for c in full["trainset"]] == 2 * ["codon_fill_holes_guided"] + 2 * (["codon_code_range"] + 2 * ["codon_stretch_codes"])
    assert "codon_fill_holes" in [c[0] for c in want["u8"]["degrade_fill"]]
    for fmt in A.FORMATS:
        assert len({want[fmt][c]["pool_sha256"] for c in A.COMBOS}) == len(A.COMBOS)
        assert len({want[fmt][c]["serial_input_sha256"] for c in A.COMBOS}) == len(A.COMBOS)
