"""The launch forms of the stem / head stencils and the CAC gate passes, as the library states them (test infrastructure, CPU only).

The launchers pick a kernel instantiation from the problem size.  A test states WHICH form it runs as a premise
(`assert head_form(...)["name"] == "head<4,4,4>"`) and places its windows and impulses on that form's seams; no result depends
on anything here.  Every rule is ASKED of the library: codon_launch_form (include/codon_hip.h) is the host functions the
launchers themselves switch on (codon_amd/csrc/launch_rules.h, px8.h), called without a launch.  Nothing of
a rule is restated here: a threshold that moves in csrc/ moves these answers, and the premises fail.  What remains is
geometry: spans, seams and probes built from the answers.

  head_form    CODON_FORM_HEAD: VEC, R, DEPTH of head_kernel (fp32) or R of head_c8_kernel, output columns per wave
  stem_form    CODON_FORM_STEM: pixels per thread; 16-bit: columns of one row per wave
  stats_form   CODON_FORM_CAC_STATS: pixels per tile, tiles per image, vector or scalar accesses
  bwd_gate_walk  CODON_FORM_CAC_BWD_GATE: tiles per image, slices, tiles per slice
  spatial_tiles  CODON_FORM_CAC_SPATIAL_FWD / _BWD: the tile edge of each kernel
  wgrad1_plan  CODON_FORM_CONV1CH_WGRAD: rows per band, pixels per chunk
  PX_TILE      the backward's pixels per tile (a module attribute, read from the library)"""
from __future__ import annotations

import ctypes as C

import torch

from codon_amd import _lib as L

_cdiv = lambda a, b: (a + b - 1) // b
_DT = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}


def ask(op: int, dtype, B: int, H: int, W: int, aligned: bool = True) -> L.Form:
    """codon_launch_form's answer for one launch."""
    f = L.Form()
    L.check(L.load().codon_launch_form(op, _DT[dtype], B, H, W, int(aligned), C.byref(f)), "codon_launch_form")
    return f


def _px_tile() -> int:
    """Pixels per tile of the 8-pixels-per-thread passes (px8.h)."""
    return ask(L.FORM_CAC_BWD_GATE, torch.float32, 1, 1, 1).tile


def __getattr__(name):
    if name == "PX_TILE":
        return _px_tile()
    raise AttributeError(name)


def _is16(dtype) -> bool:
    return dtype in (torch.bfloat16, torch.float16)


def _spans(n: int, step: int) -> list:
    return [(i, min(i + step, n)) for i in range(0, n, step)]


def head_form(dtype, B: int, H: int, W: int, aligned: bool = True) -> dict:
    """name, rows (R: rows per band), seg_cols (output columns per wave), bands = [(first row, one past the last)],
    segs = [(first column, one past the last)].  aligned: x, y and res start on 16 bytes (torch allocations do)."""
    f = ask(L.FORM_HEAD, dtype, B, H, W, aligned)
    args = (f.rows,) if _is16(dtype) else (f.vec, f.rows) + ((f.depth,) if f.depth != 1 else ())
    name = ("head_c8<%s>" if _is16(dtype) else "head<%s>") % ",".join(map(str, args))
    return {"name": name, "rows": f.rows, "seg_cols": f.cols, "bands": _spans(H, f.rows), "segs": _spans(W, f.cols), "H": H, "W": W}


def stem_form(dtype, B: int, H: int, W: int, aligned: bool = True) -> dict:
    """name, vec, segs and starts.  The fp32 kernels give a thread VEC consecutive pixels of one row and a workgroup 256
    consecutive threads of the flattened (b, y, x / VEC) index: no column segments; `starts` are the pixels (b, y, x) at
    which the second, a middle and the last workgroup begin.  The 16-bit kernel gives a wave a segment of columns of one row."""
    f = ask(L.FORM_STEM, dtype, B, H, W, aligned)
    vec, starts = f.vec, []
    if f.cols:
        return {"name": f"stem_c8<{vec}>", "vec": vec, "segs": _spans(W, f.cols), "starts": starts, "H": H, "W": W}
    wv = W // vec
    nblk = _cdiv(B * H * wv, 256)
    for m in sorted({1, nblk // 2, nblk - 1} - {0}):
        if m < nblk:
            idx = 256 * m
            starts.append((idx // wv // H, idx // wv % H, idx % wv * vec))
    return {"name": f"stem<{vec}>", "vec": vec, "segs": [(0, W)], "starts": starts, "H": H, "W": W}


def stats_form(H: int, W: int, aligned: bool = True) -> dict:
    """name, tile (pixels of the flattened plane per workgroup), ntiles, last (pixels in the last tile)."""
    f = ask(L.FORM_CAC_STATS, torch.float32, 1, H, W, aligned)
    name = f"stats<{f.tile},v{4 if f.vector else 1}>" if f.tile == _px_tile() else f"stats_small<{f.tile}>"
    return {"name": name, "tile": f.tile, "ntiles": f.tiles, "last": H * W - (f.tiles - 1) * f.tile}


def bwd_gate_walk(H: int, W: int) -> dict:
    """ntiles (the backward's tiles per image), per, and the tile range [k0, k1) each slice of the gate kernel walks."""
    f = ask(L.FORM_CAC_BWD_GATE, torch.float32, 1, H, W)
    nt, per = f.tiles, f.per
    sl = [(min(s * per, nt), min(s * per + per, nt)) for s in range(f.slices)]
    return {"ntiles": nt, "per": per, "slices": sl, "last": H * W - (nt - 1) * f.tile}


def spatial_tiles(H: int, W: int, backward: bool = False) -> dict:
    t = ask(L.FORM_CAC_SPATIAL_BWD if backward else L.FORM_CAC_SPATIAL_FWD, torch.float32, 1, H, W).tile
    return {"rows": _spans(H, t), "cols": _spans(W, t)}


def wgrad1_plan(H: int, W: int) -> dict:
    f = ask(L.FORM_CONV1CH_WGRAD, torch.float32, 1, H, W)
    return {"bands": _spans(H, f.rows), "chunks": _spans(W, f.cols)}


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
