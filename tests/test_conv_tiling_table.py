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


@pytest.mark.parametrize("geo,B", sorted(CB.BATCH_TILING))
def test_batches_of_the_small_image_take_the_tilings_they_are_there_for(geo, B):
    """The premises of tests/test_gpu_f32_tilings.py, for every conv form, chained and plain, outside and inside a pair
    bracket: a change of f32_tiling's constants fails here, without a GPU."""
    CB.assert_batch_tiling(geo, B)


def test_the_small_image_reaches_every_tiling_in_every_kind_of_launch():
    """Each geometry: the chained conv and a plain 5x5 run in all four tilings, a 3x3 in its three and a 1x1 in its two; geometry
    A's pair batches hold a padded and an unpadded cout-split pair, a batch that is SPLIT outside and SOLO inside a bracket,
    and a SOLO pair."""
    for geo in CB.GEOMETRY:
        single = [v[0] for (g, _), v in CB.BATCH_TILING.items() if g == geo]
        for i in range(2):
            assert {t[i] for t in single} == {CB.T8, CB.T4, CB.SOLO, CB.SPLIT}, (geo, i)
        assert {t[2] for t in single} == {CB.T8, CB.SOLO, CB.SPLIT}, geo  # 3x3 and 1x1 keep 8 x 32 at every larger grid
        assert {t[3] for t in single} == {CB.T8, CB.SOLO}, geo            # ... and a 1x1 never splits its couts
    H, W = CB.GEOMETRY["A"]
    split_wgs = lambda B: 2 * B * ((H + 1) // 2) * ((W + 31) // 32)       # both launches of a pair, 2 x 32 tiles
    assert CB.BATCH_TILING["A", 5][1][1] == CB.BATCH_TILING["A", 8][1][1] == CB.SPLIT
    assert split_wgs(5) <= CB.PAIR_GRID_LIMIT < split_wgs(8)
    assert CB.BATCH_TILING["A", 12][0][:3] == (CB.SPLIT,) * 3 and CB.BATCH_TILING["A", 12][1] == (CB.SOLO,) * 4
    assert CB.BATCH_TILING["A", 17][1] == (CB.SOLO,) * 4
