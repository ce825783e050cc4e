"""codon_launch_form, asked through tests/forms.py over a grid of shapes, the three dtypes and aligned / misaligned operands,
returns the table that tests/golden/launch_forms.json holds.  The table was recorded with tests/form_table.py
(python -m tests.form_table OUT.json) on the commit before forms.py asked the library, when it restated the launchers in
Python: the rules the launchers and the query now share are the rules that mirror held, at every threshold from both sides.
A threshold that moves in csrc/launch_rules.h fails here and names the case.  Host arithmetic only, no GPU."""
import json
import math
import os

import pytest

from tests import form_table as FT


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "launch_forms.json")) as f:
        return json.load(f)


def test_the_golden_covers_the_grid(golden):
    assert sorted(golden) == sorted(FT._key(s) for s in FT.SHAPES)
    names = {v[0] for row in golden.values() for k in ("stem", "head", "stats") for v in row[k].values()}
    assert names == {"head<1,1,16>", "head<4,4,4>", "head<1,4,8>", "head<4,16>", "head<1,4>", "head_c8<4>", "head_c8<8>",
                     "stem<1>", "stem<4>", "stem_c8<2>", "stats_small<256>", "stats<2048,v4>", "stats<2048,v1>"}    # every form occurs
    px = lambda k: math.prod(int(v) for v in k.split("x"))
    # both sides of every threshold
    assert {65535, 65536, 65537} <= {px(k) for k in golden} and {(1 << 22) - 1028, (1 << 22) - 1, 1 << 22} <= {px(k) for k in golden}
    assert {32767, 32768, 32769} <= {px(k.split("x", 1)[1]) for k in golden}
    assert {1, 2, 8, 9, 33} <= {row["walk"][0] for row in golden.values()}


def test_launch_forms_are_the_recorded_ones(golden):
    table = json.loads(json.dumps(FT.table()))
    cells = lambda row: {(op, k): v for op, r in row.items() for k, v in (r.items() if isinstance(r, dict) else [("", r)])}
    wrong = [f"{shape} {op} {k}: got {cells(table[shape])[op, k]}, recorded {v}" for shape, row in sorted(golden.items())
             for (op, k), v in cells(row).items() if cells(table[shape])[op, k] != v]
    assert not wrong, f"{len(wrong)} cells differ:\n" + "\n".join(wrong[:16])
