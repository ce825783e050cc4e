"""codon_conv_tiling_f32 over a grid of batches, image sizes, conv forms and both sides of a pair bracket returns the table
that tests/golden/f32_tiling.json holds.  The table was recorded with tests/conv_bits.py (python -m
tests.conv_bits tiling OUT.json) from the library of the commit before the fp32 launchers were moved onto one tiling
function: the rule they and the query now share is the rule the launchers had.  Host arithmetic only, no GPU."""
import json
import os

import pytest

from tests import conv_bits as CB


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "f32_tiling.json")) as f:
        return json.load(f)


def test_the_golden_covers_the_grid(golden):
    assert sorted(golden) == sorted(f"k{k}_{ci}_{co}_chained{ch}_pair{p}" for k, ci, co, ch in CB.TILING_FORMS for p in (0, 1))
    assert all(len(v) == len(CB.TILING_BATCH) * len(CB.TILING_HW) and set(v) <= set("0123") for v in golden.values())
    assert set("".join(golden.values())) == set("0123")                 # every tiling occurs


def test_tiling_table_is_the_recorded_one(golden):
    table = CB.tiling_table()
    for key in sorted(golden):
        assert table[key] == golden[key], key


@pytest.mark.parametrize("B,H,W", CB.FWD_SHAPES)
def test_bit_test_shapes_take_the_tilings_they_are_there_for(B, H, W):
    CB.assert_fwd_tiling(B, H, W)
