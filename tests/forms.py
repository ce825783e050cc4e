"""The launch forms of the stem / head stencils and the CAC gate passes, restated (test infrastructure, CPU only).

The launchers pick a kernel instantiation from the problem size.  A test states WHICH form it runs as a premise
(`assert head_form(...)["name"] == "head<4,4,4>"`) and places its windows and impulses on that form's seams; no result depends
on anything here.  A mirror kept in step by hand, as tests/bounds.py::wgrad_bands is:

  head_form    codon_amd/csrc/stencil.hip head_launch (the B H W <= 65536 / v4 / `big` lines) and head_launch_v (nband, nseg);
               codon_amd/csrc/ew_c8.hip head_fwd_c8 (`big`) and head_c8_launch (nseg: 62 output columns per wave)
  stem_form    stencil.hip stem_launch / stem_pair_fwd (`tiny`, `v4`); ew_c8.hip stem_c8_launch (VEC = 2, 128 columns per wave)
  stats_form   codon_amd/csrc/cac.hip STATS_SMALL_HW, STATS_SMALL_TILE, cac_stats_tiles; px8.h PX_TILE and px_dispatch
  bwd_gate_walk  codon_amd/csrc/cac_bwd.hip cac_bwd_tiles and the k0 / k1 lines of cac_bwd_gate_kernel (GATE_SLICES)
  spatial_tiles  cac.hip SPF_T / cac_bwd.hip SPB_T: 32 x 32 pixel tiles
  wgrad1_plan  stencil.hip W1_ROWS and the 64-pixel chunk loop of conv1ch_wgrad_kernel (ew_c8.hip W1C8_ROWS: the same 8)"""
from __future__ import annotations

import torch

HEAD_TINY_PIXELS = 65536          # stencil.hip: B H W <= 65536 -> one row and 64 pixels per wave
HEAD_BIG_PIXELS = 1 << 22         # stencil.hip / ew_c8.hip: `big`
STATS_SMALL_HW = 32768            # cac.hip
STATS_SMALL_TILE = 256            # cac.hip
PX_TILE = 2048                    # px8.h
GATE_SLICES = 8                   # cac_bwd.hip
SPATIAL_TILE = 32                 # cac.hip SPF_T, cac_bwd.hip SPB_T
W1_ROWS = 8                       # stencil.hip, ew_c8.hip
W1_CHUNK = 64

_cdiv = lambda a, b: (a + b - 1) // b


def _is16(dtype) -> bool:
    return dtype in (torch.bfloat16, torch.float16)


def _spans(n: int, step: int) -> list:
    return [(i, min(i + step, n)) for i in range(0, n, step)]


def head_form(dtype, B: int, H: int, W: int, aligned: bool = True) -> dict:
    """name, rows (R: rows per band), seg_cols (output columns per wave), bands = [(first row, one past the last)],
    segs = [(first column, one past the last)].  aligned: x, y and res start on 16 bytes (torch allocations do)."""
    px = B * H * W
    big = px >= HEAD_BIG_PIXELS
    if _is16(dtype):
        R, cols = (8 if big else 4), 62
        name = f"head_c8<{R}>"
    elif px <= HEAD_TINY_PIXELS:
        R, cols, name = 1, 64, "head<1,1,16>"
    elif W % 4 == 0 and aligned:
        R, cols = (16 if big else 4), 256
        name = "head<4,16>" if big else "head<4,4,4>"
    else:
        R, cols = 4, 64
        name = "head<1,4>" if big else "head<1,4,8>"
    return {"name": name, "rows": R, "seg_cols": cols, "bands": _spans(H, R), "segs": _spans(W, cols), "H": H, "W": W}


def stem_form(dtype, B: int, H: int, W: int, aligned: bool = True) -> dict:
    """name, vec, segs and starts.  The fp32 kernels give a thread VEC consecutive pixels of one row and a workgroup 256
    consecutive threads of the flattened (b, y, x / VEC) index: no column segments; `starts` are the pixels (b, y, x) at
    which the second, a middle and the last workgroup begin.  The 16-bit kernel gives a wave 128 columns of one row."""
    if _is16(dtype):
        return {"name": "stem_c8<2>", "vec": 2, "segs": _spans(W, 128), "starts": [], "H": H, "W": W}
    v4 = B * H * W > HEAD_TINY_PIXELS and W % 4 == 0 and aligned
    vec = 4 if v4 else 1
    wv = W // vec
    nblk = _cdiv(B * H * wv, 256)
    starts = []
    for m in sorted({1, nblk // 2, nblk - 1} - {0}):
        if m < nblk:
            idx = 256 * m
            starts.append((idx // wv // H, idx // wv % H, idx % wv * vec))
    return {"name": f"stem<{vec}>", "vec": vec, "segs": [(0, W)], "starts": starts, "H": H, "W": W}


def stats_form(H: int, W: int, aligned: bool = True) -> dict:
    """name, tile (pixels of the flattened plane per workgroup), ntiles, last (pixels in the last tile)."""
    HW = H * W
    if HW <= STATS_SMALL_HW:
        name, tile = "stats_small<256>", STATS_SMALL_TILE
    else:
        name, tile = ("stats<2048,v4>" if HW % 4 == 0 and aligned else "stats<2048,v1>"), PX_TILE
    nt = _cdiv(HW, tile)
    return {"name": name, "tile": tile, "ntiles": nt, "last": HW - (nt - 1) * tile}


def bwd_gate_walk(H: int, W: int) -> dict:
    """ntiles (2048-pixel tiles of the backward), per, and the tile range [k0, k1) each of the 8 slices walks."""
    nt = _cdiv(H * W, PX_TILE)
    per = _cdiv(nt, GATE_SLICES)
    sl = [(min(s * per, nt), min(s * per + per, nt)) for s in range(GATE_SLICES)]
    return {"ntiles": nt, "per": per, "slices": sl, "last": H * W - (nt - 1) * PX_TILE}


def spatial_tiles(H: int, W: int) -> dict:
    return {"rows": _spans(H, SPATIAL_TILE), "cols": _spans(W, SPATIAL_TILE)}


def wgrad1_plan(H: int, W: int) -> dict:
    return {"bands": _spans(H, W1_ROWS), "chunks": _spans(W, W1_CHUNK)}


def seam_lines(spans: list, n: int, reach: int = 0) -> list:
    """Indices on each side of every seam of `spans`, the first and last index, and (reach > 0) the ones `reach` further in
    on both sides; sorted, unique, inside [0, n)."""
    s = {0, n - 1}
    for a, _ in spans[1:]:
        s |= {a - 1, a, a - 1 - reach, a + reach}
    return sorted(i for i in s if 0 <= i < n)


def where(form: dict, h: int, w: int, rows_key: str = "bands", cols_key: str = "segs") -> str:
    """'band j (rows a..b), segment s (columns c..d)' of pixel (h, w): for failure messages."""
    j = next(i for i, (a, b) in enumerate(form[rows_key]) if a <= h < b)
    s = next(i for i, (a, b) in enumerate(form[cols_key]) if a <= w < b)
    (ra, rb), (ca, cb) = form[rows_key][j], form[cols_key][s]
    return (f"band {j} of {len(form[rows_key])} (rows {ra}..{rb - 1}), segment {s} of {len(form[cols_key])} "
            f"(columns {ca}..{cb - 1})")


def pack_probes(pix: list, reach: int, per_round: int) -> list:
    """Rounds of at most per_round probe pixels (b, h, w) such that no two of a round lie in the same image within `reach`
    pixels of each other on both axes (their (reach + 1)-wide footprints do not overlap).  Greedy, order preserving."""
    rounds = []
    for p in dict.fromkeys(pix):
        for r in rounds:
            if len(r) < per_round and all(q[0] != p[0] or abs(q[1] - p[1]) > reach or abs(q[2] - p[2]) > reach for q in r):
                r.append(p)
                break
        else:
            rounds.append([p])
    return rounds


def probe_pixels(B: int, H: int, W: int, row_spans: list, col_spans: list, max_lines: int = 12) -> list:
    """(b, h, w) probes: the four corners, and every seam row crossed with every seam column (both sides of each; the first
    `max_lines` seam rows / columns around the first, a middle and the last seam when there are more), over the first and
    the last image alternately."""
    def pick(spans, n):
        lines = seam_lines(spans, n)
        if len(lines) <= max_lines:
            return lines
        seams = [a for a, _ in spans[1:]]
        keep = {0, n - 1}
        for a in (seams[0], seams[len(seams) // 2], seams[-1]):
            keep |= {a - 1, a}
        return sorted(keep)
    rows, cols = pick(row_spans, H), pick(col_spans, W)
    pix = [(0, 0, 0), (B - 1, 0, W - 1), (0, H - 1, 0), (B - 1, H - 1, W - 1)]
    for i, h in enumerate(rows):
        for j, w in enumerate(cols):
            pix.append(((B - 1) if (i + j) % 2 else 0, h, w))
    return list(dict.fromkeys(pix))
