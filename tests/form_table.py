"""tests/forms.py over a grid of shapes, the three dtypes and aligned / misaligned operands, as a table (test infrastructure,
CPU only).  tests/golden/launch_forms.json is this table as recorded on the commit before forms.py asked the library
(python -m tests.form_table OUT.json), when it was a pure-Python mirror of the launchers kept in step by hand;
tests/test_launch_form_table.py holds the library's answers to it.  Only the public helpers of tests/forms.py are used, so
the module runs unchanged on that older tree.

The grid straddles every threshold from both sides, by batch and by image size:
  tiny  65535 / 65536 / 65537 pixels, with W % 4 zero and non-zero, reached by one image and by batches of smaller ones
  big   2^22 - 1028, 2^22 - 1, 2^22 and above, likewise
  stats H W = 32767 / 32768 / 32769 (99 x 331), alone and in a batch (the rule looks at H W only)
  px    W % 4 and H W % 4 zero and non-zero, independently
  gate  one, two, eight and nine 2048-pixel tiles of the backward (slices of one tile, then of two), 33 tiles (an empty slice)"""
import json
import sys

import torch

from tests import forms

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SHAPES = [
    (1, 1, 1), (2, 19, 45), (1, 16, 64), (1, 32, 64), (2, 50, 41), (1, 128, 128), (1, 129, 128), (1, 9, 125),
    # tiny: <= 65536 pixels
    (1, 1, 65535), (1, 1, 65536), (1, 1, 65537), (1, 255, 257), (1, 256, 256), (1, 16385, 4), (1, 257, 256), (1, 128, 512),
    (2, 128, 256), (3, 128, 256), (4, 64, 256), (5, 64, 256), (16, 64, 64), (17, 64, 64), (1, 64, 96),
    # the stats threshold: H W <= 32768
    (1, 217, 151), (1, 128, 256), (1, 99, 331), (1, 8193, 4), (4, 99, 331),
    # mid: W % 4 and H W % 4
    (1, 253, 260), (2, 127, 261), (1, 256, 258), (1, 370, 463), (3, 300, 256), (1, 480, 640),
    # big: >= 2^22 pixels
    (1, 1048319, 4), (1, 4079, 1028), (1, 2047, 2049), (1, 2048, 2048), (4, 1024, 1024), (3, 1024, 1024), (5, 1024, 1024), (4, 1024, 1023),
    (4, 1025, 1028), (4, 1025, 1027), (32, 480, 640), (64, 256, 256), (63, 256, 256),
]


def _key(shape):
    return "x".join(map(str, shape))


def table():
    """{shape: {"stem" / "head": {dtype_aligned: [...]}, "stats": {aligned: [...]}, "walk", "spatial", "wgrad1"}}"""
    out = {}
    for shape in SHAPES:
        B, H, W = shape
        row = {"stem": {}, "head": {}, "stats": {}}
        for dn, dt in DTYPES.items():
            for al in (True, False):
                k = f"{dn}_{'aligned' if al else 'misaligned'}"
                s, h = forms.stem_form(dt, B, H, W, al), forms.head_form(dt, B, H, W, al)
                row["stem"][k] = [s["name"], s["vec"], len(s["segs"]), s["segs"][0][1], [list(p) for p in s["starts"]]]
                row["head"][k] = [h["name"], h["rows"], h["seg_cols"], len(h["bands"]), len(h["segs"])]
        for al in (True, False):
            s = forms.stats_form(H, W, al)
            row["stats"]["aligned" if al else "misaligned"] = [s["name"], s["tile"], s["ntiles"], s["last"]]
        w = forms.bwd_gate_walk(H, W)
        row["walk"] = [w["ntiles"], w["per"], [list(p) for p in w["slices"]], w["last"]]
        t, p = forms.spatial_tiles(H, W), forms.wgrad1_plan(H, W)
        row["spatial"] = [len(t["rows"]), t["rows"][0][1], len(t["cols"]), t["cols"][0][1]]
        row["wgrad1"] = [len(p["bands"]), p["bands"][0][1], len(p["chunks"]), p["chunks"][0][1]]
        out[_key(shape)] = row
    return out


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(table(), f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")
