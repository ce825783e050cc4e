"""Registration of a depth sensor's maps to the colour camera: the sensor's own depth file plus the rig's
calibration in, the map on the colour camera's grid out -- at the colour resolution (a --train-depth target, a --label) or at
colour / scale, which is what `infer --lr-depth`, `train --train-lr-depth` and `--val-lr-depth` read.  Disocclusion holes come
out as code 0, which `--fill-holes --fill-guided` was built for.

    python -m codon_amd.register --depth DIR --calib FILE --out DIR [--scale {1,4,8,16}] [--depth-bits {8,16}] [--depth-max N]
                                 [--depth-unit M] [--radial] [--stats] [--clean [--clean-tolerance CODES]
                                 [--clean-tolerance-rel F] [--clean-min-support K] [--clean-min-region N]]
                                 [--smooth [--smooth-radius R] [--smooth-passes P] [--smooth-sigma S] [--smooth-tolerance CODES]
                                 [--smooth-tolerance-rel F] [--smooth-no-pairs]]
                                 [--temporal [--temporal-window W] [--temporal-causal] [--temporal-tolerance CODES]
                                 [--temporal-tolerance-rel F] [--temporal-min-count M] [--temporal-min-fill F]]

A z-buffered forward projection in integers (tests/register_ref.py; csrc/register.hip): every valid source pixel's four corners
are projected, the box of them takes the pixel's z in the colour camera's frame under a minimum.  Only the tables -- the corner
rays with the lens distortion removed and the rotation applied, the translation, the projection -- are floating point, float64
on the host, once.  Not handled here: distortion of the COLOUR lens (undistort the colour images first, with
`python -m codon_amd.undistort`, whose --calib-out is the calibration to pass here: DESIGN 12.16), a rolling shutter, and the
growth of a foreground silhouette by up to one target pixel (the box is conservative).  --clean removes the sensor's flying
pixels and speckles first, in the sensor's frame (codon_amd.clean): the same bytes as `python -m codon_amd.clean`
followed by this, on one upload.  --smooth then smooths what is left, still in the sensor's frame (codon_amd.smooth):
the same bytes as `python -m codon_amd.smooth` between the two.  --temporal takes the files of --depth, in the order of their names, as ONE sequence of a
camera that stands still and filters it over time first of all (codon_amd.temporal's TemporalStream): every file
is uploaded once and goes stream -> (cleaner) -> (smoother) -> registration on the device, and the bytes are those of `python -m
codon_amd.temporal`, then clean where --clean is given, then smooth where --smooth is given, then this, run as separate commands:
the recommended order, temporal -> clean -> smooth -> register."""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import math
import os

import numpy as np
import torch

from . import _lib as L
from . import clean as cleaning
from . import codes as K
from . import ops
from . import smooth as smoothing
from . import temporal as filtering

A_LIMIT, T_LIMIT, F_LIMIT, C_LIMIT = 1 << 22, 1 << 38, 1 << 20, 1 << 21
UNDISTORT_ITERS = 40
SCALES = (1, 4, 8, 16)
MAX_SIDE = 4096
STATS = ("valid", "outside", "dropped", "filled")


def _finite(who: str, what: str, values):
    try:
        v = [float(x) for x in values]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {what} {values!r} is not a list of numbers") from None
    if not all(math.isfinite(x) for x in v):
        raise ValueError(f"{who}: {what} {values!r} is not finite")
    return v


@dataclasses.dataclass(frozen=True)
class Camera:
    """A pinhole camera with Brown distortion (k1, k2, p1, p2, k3): pixel centres at integer coordinates"""
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    dist: tuple = (0.0,) * 5

    def __post_init__(self):
        who = "Camera"
        for n in ("width", "height"):
            K.integer(who, n, getattr(self, n), 1, MAX_SIDE, f"an integer in 1..{MAX_SIDE}")
        fx, fy, cx, cy = _finite(who, "fx, fy, cx, cy", (self.fx, self.fy, self.cx, self.cy))
        if fx <= 0 or fy <= 0:
            raise ValueError(f"{who}: focal lengths {self.fx!r}, {self.fy!r} must be positive")
        d = self.dist
        if not isinstance(d, (list, tuple, np.ndarray)) or len(d) != 5:
            raise ValueError(f"{who}: dist {d!r} (five numbers: k1, k2, p1, p2, k3)")
        object.__setattr__(self, "dist", tuple(_finite(who, "dist", d)))
        for n, v in (("fx", fx), ("fy", fy), ("cx", cx), ("cy", cy)):
            object.__setattr__(self, n, v)

    @classmethod
    def from_mapping(cls, m, name="camera"):
        if not isinstance(m, dict):
            raise ValueError(f"Calibration: {name} must be a mapping")
        missing = [k for k in ("width", "height", "fx", "fy", "cx", "cy") if k not in m]
        if missing:
            raise ValueError(f"Calibration: {name} lacks {', '.join(missing)}")
        return cls(m["width"], m["height"], m["fx"], m["fy"], m["cx"], m["cy"], tuple(m.get("dist", (0.0,) * 5)))


@dataclasses.dataclass(frozen=True)
class Calibration:
    """A rig: the depth camera, the colour camera, and the depth -> colour rigid motion X_c = rotation X_d + translation (metres)"""
    depth: Camera
    color: Camera
    rotation: tuple
    translation: tuple

    def __post_init__(self):
        who = "Calibration"
        if not isinstance(self.depth, Camera) or not isinstance(self.color, Camera):
            raise ValueError(f"{who}: depth and color must be Camera records")
        try:
            rows = [list(r) for r in self.rotation]
        except TypeError:
            rows = []
        if len(rows) != 3 or any(len(r) != 3 for r in rows):
            raise ValueError(f"{who}: rotation must be 3 x 3 (depth -> colour)")
        R = np.array([_finite(who, "rotation", r) for r in rows], dtype=np.float64)
        if np.abs(R.T @ R - np.eye(3)).max() > 1e-6:
            raise ValueError(f"{who}: rotation is not orthonormal (|R^T R - I| = {np.abs(R.T @ R - np.eye(3)).max():.3g} > 1e-6)")
        try:
            t = list(self.translation)
        except TypeError:
            t = []
        if len(t) != 3:
            raise ValueError(f"{who}: translation must be three numbers (metres)")
        t = _finite(who, "translation", t)
        if any(self.color.dist):
            raise ValueError(f"{who}: color.dist {self.color.dist!r} is not zero: undistort the colour images first "
                             "(python -m codon_amd.undistort --calib-out ...)")
        object.__setattr__(self, "rotation", tuple(tuple(float(v) for v in r) for r in R))
        object.__setattr__(self, "translation", tuple(t))

    @classmethod
    def from_mapping(cls, m):
        if not isinstance(m, dict):
            raise ValueError("Calibration: the calibration must be a mapping")
        missing = [k for k in ("depth", "color", "rotation", "translation") if k not in m]
        if missing:
            raise ValueError(f"Calibration: missing {', '.join(missing)}")
        return cls(Camera.from_mapping(m["depth"], "depth"), Camera.from_mapping(m["color"], "color"), m["rotation"], m["translation"])

    @classmethod
    def from_json(cls, path):
        with open(path) as fh:
            try:
                m = json.load(fh)
            except json.JSONDecodeError as e:
                raise ValueError(f"Calibration: {path}: {e}") from None
        return cls.from_mapping(m)


# ---- the tables: numpy on the host, float64, once (tests/register_ref.py restates them) --------------------------------------------

def distort(x, y, dist):
    """The Brown model on normalised coordinates"""
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return x * rad + dx, y * rad + dy


def undistort(xd, yd, dist):
    """`distort` undone by UNDISTORT_ITERS fixed-point iterations x <- (x_d - tangential(x)) / radial(x)"""
    k1, k2, p1, p2, k3 = dist
    x, y = xd.copy(), yd.copy()
    for _ in range(UNDISTORT_ITERS):
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (xd - dx) / rad, (yd - dy) / rad
    return x, y


def corner_rays(cam: Camera, radial: bool = False) -> np.ndarray:
    """(height + 1, width + 1, 3) float64: the undistorted normalised ray of the image point (j - 0.5, i - 0.5), the top-left
    corner of pixel (i, j) -- (x_n, y_n, 1), or that over its length for a file of ranges along the ray"""
    j, i = np.meshgrid(np.arange(cam.width + 1, dtype=np.float64), np.arange(cam.height + 1, dtype=np.float64))
    x, y = undistort((j - 0.5 - cam.cx) / cam.fx, (i - 0.5 - cam.cy) / cam.fy, cam.dist)
    r = np.stack([x, y, np.ones_like(x)], axis=-1)
    if radial:
        r = r / np.sqrt((r * r).sum(axis=-1, keepdims=True))
    return r


def ray_table(cal: Calibration, radial: bool = False) -> np.ndarray:
    """A: int32 (hs + 1, ws + 1, 3), rint(2^20 R r) of the depth camera's corner rays; an entry of 2^22 or more in magnitude (a
    lens model that folds over, a field of view beyond 150 degrees) is refused by name"""
    r = corner_rays(cal.depth, radial)
    a = np.rint(float(1 << 20) * (r @ np.asarray(cal.rotation, dtype=np.float64).T))
    if not np.isfinite(a).all() or np.abs(a).max() >= A_LIMIT:
        raise ValueError("ray_table: a corner ray of 2^22 or more in Q20 (|x_n| or |y_n| of 4 or more): the depth camera's "
                         "intrinsics or distortion do not describe a lens this can register")
    return a.astype(np.int32)


def translation_q20(cal: Calibration, unit: float) -> np.ndarray:
    """T: int64[3], rint(2^20 t / unit) with t in metres and unit in metres per code"""
    u = K.positive("translation_q20", "depth_unit", unit, "a positive number of metres per code")
    v = np.rint(float(1 << 20) * np.asarray(cal.translation, dtype=np.float64) / u)
    if not np.isfinite(v).all() or np.abs(v).max() >= T_LIMIT:
        raise ValueError(f"translation_q20: a translation of {cal.translation!r} m is 2^18 codes or more at {u!r} m per code")
    return v.astype(np.int64)


def projection_q8(cal: Calibration, scale: int) -> np.ndarray:
    """FX, FY, CX, CY: int32[4] in Q8 pixels of the colour grid reduced by `scale`: FX = rint(256 fx / s),
    CX = rint(256 ((cx + 0.5) / s - 0.5))"""
    if scale not in SCALES:
        raise ValueError(f"projection_q8: scale {scale!r} (1, 4, 8 or 16)")
    c, s = cal.color, float(scale)
    p = [np.rint(256.0 * c.fx / s), np.rint(256.0 * c.fy / s), np.rint(256.0 * ((c.cx + 0.5) / s - 0.5)),
         np.rint(256.0 * ((c.cy + 0.5) / s - 0.5))]
    if not (1 <= p[0] < F_LIMIT and 1 <= p[1] < F_LIMIT):
        raise ValueError(f"projection_q8: focal lengths {c.fx!r}, {c.fy!r} at scale {scale} are not 1 .. 2^20 - 1 in Q8 pixels")
    if not (abs(p[2]) < C_LIMIT and abs(p[3]) < C_LIMIT):
        raise ValueError(f"projection_q8: principal point {c.cx!r}, {c.cy!r} at scale {scale} is 2^21 or more in Q8 pixels")
    return np.array(p, dtype=np.int32)


# ---- the device side ----------------------------------------------------------------------------------------------------------------

class Registration:
    """A rig's tables on the device.  reg(codes) registers a batch of the depth camera's planes to the colour camera's grid at
    colour / scale.  depth_unit: metres per code; radial: the file holds ranges along the ray, not z."""

    def __init__(self, cal: Calibration, scale: int = 1, depth_unit: float = 0.001, radial: bool = False, device=None):
        if not isinstance(cal, Calibration):
            raise ValueError("Registration: cal must be a Calibration")
        self.cal, self.scale, self.depth_unit, self.radial = cal, scale, depth_unit, bool(radial)
        self.proj = projection_q8(cal, scale)
        self.trans = translation_q20(cal, depth_unit)
        self.out_size = (cal.color.height // scale, cal.color.width // scale)
        if min(self.out_size) < 1:
            raise ValueError(f"Registration: a {cal.color.height}x{cal.color.width} colour image leaves nothing at scale {scale}")
        rays = ray_table(cal, self.radial)
        self.device = torch.device("cuda:0" if device is None else device)
        self.rays = torch.from_numpy(rays).to(self.device)
        self._trans = (C.c_int64 * 3)(*(int(v) for v in self.trans))
        self._proj = (C.c_int32 * 4)(*(int(v) for v in self.proj))

    def __call__(self, codes: torch.Tensor, depth_max: int = None, stats: bool = False):
        """codes: (h, w) or (B, h, w) uint8 codes, or u16 codes as int16 / uint16, of the depth camera's size, 0 a hole, on this
        object's device -> codes of shape (..., ho, wo) in the argument's dtype, z in the colour camera's frame, 0 where nothing
        landed; the argument is not modified.  stats=True: (codes, int32 (B, 4) on the device: valid source pixels, pixels wholly
        outside the plane, dropped pixels, filled target pixels).  Three launches; no host synchronisation."""
        who = "register_depth"
        p = K.code_planes(who, codes, depth_max)
        d = self.cal.depth
        if (p.h, p.w) != (d.height, d.width):
            raise ValueError(f"{who}: a {p.h}x{p.w} plane, and the depth camera of the calibration is {d.height}x{d.width}")
        dev = p.dev
        if dev != self.rays.device:
            raise RuntimeError(f"{who}: codes on {dev}, the tables on {self.rays.device}")
        ho, wo = self.out_size
        out = p.out(ho, wo)
        counts = torch.empty((p.B, 4), dtype=torch.int32, device=dev) if stats else None
        P_ = C.c_void_p
        with ops._on(dev):
            ws = K.workspace(who, "codon_register_workspace_bytes", dev, p.B, ho, wo)
            L.check(L.load().codon_register_depth(p.B, p.h, p.w, p.ptr, p.fmt, p.top,
                                                  P_(self.rays.data_ptr()), self._trans, self._proj, ho, wo, P_(out.data_ptr()),
                                                  P_(counts.data_ptr()) if stats else None, P_(ws.data_ptr()), ws.numel(),
                                                  ops._stream(dev)), who)
        return (out, counts) if stats else out


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m codon_amd.register", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", required=True, metavar="DIR", help="the sensor's depth maps, in the depth camera's own frame")
    ap.add_argument("--calib", required=True, metavar="FILE", help="JSON: depth, color (width, height, fx, fy, cx, cy, dist), "
                    "rotation (3 x 3, depth -> colour), translation (metres)")
    ap.add_argument("--out", required=True, metavar="DIR", help="where the registered maps go, under the same file names")
    ap.add_argument("--scale", type=int, default=1, choices=SCALES,
                    help="1: the colour camera's grid (a --train-depth target, a --label); S: colour / S, what --lr-depth reads")
    K.add_depth_args(ap, depth_unit=0.001)
    ap.add_argument("--radial", action="store_true", help="the files hold ranges along the ray, not z")
    ap.add_argument("--stats", action="store_true", help="print valid=, outside=, dropped= and filled= per file")
    ap.add_argument("--clean", action="store_true", help="remove flying pixels and speckles first (python -m codon_amd.clean); "
                    "--stats then also prints valid=, flying=, speckle= and regions= of the cleaning")
    cleaning.add_arguments(ap, "clean-")
    ap.add_argument("--smooth", action="store_true", help="smooth the maps in the sensor's frame, after --clean (python -m codon_amd.smooth); "
                    "--stats then also prints valid=, changed=, alone= and max= of the smoothing")
    smoothing.add_arguments(ap, "smooth-")
    ap.add_argument("--temporal", action="store_true", help="the files are one sequence of a fixed camera: filter it over time first "
                    "(python -m codon_amd.temporal --stream); --stats then also prints valid=, rejected=, filled= and changed= of the filter")
    filtering.add_arguments(ap, "temporal-")
    a = ap.parse_args(argv)
    a.top = K.depth_args_of(ap, a)
    if os.path.abspath(a.out) == os.path.abspath(a.depth):
        ap.error("--out is --depth: the registered maps would overwrite the sensor's")
    a.temporal_filter = None
    if a.temporal:
        a.temporal_filter = filtering.filter_of(a, ap, "temporal-")
        if a.temporal_filter.tolerance > a.top:
            ap.error(f"--temporal-tolerance {a.temporal_filter.tolerance} is above the largest code {a.top}")
    else:
        for name, default in filtering.DEFAULTS.items():
            if getattr(a, "temporal_" + name) != default:
                ap.error(f"--temporal-{name.replace('_', '-')} needs --temporal")
    a.cleaner = None
    if a.clean:
        a.cleaner = cleaning.cleaner_of(a, ap, "clean-")
        if a.cleaner.tolerance > a.top:
            ap.error(f"--clean-tolerance {a.cleaner.tolerance} is above the largest code {a.top}")
    else:
        for name, default in cleaning.DEFAULTS.items():
            if getattr(a, "clean_" + name) != default:
                ap.error(f"--clean-{name.replace('_', '-')} needs --clean")
    a.smoother = None
    if a.smooth:
        a.smoother = smoothing.smoother_of(a, ap, "smooth-")
        if a.smoother.tolerance > a.top:
            ap.error(f"--smooth-tolerance {a.smoother.tolerance} is above the largest code {a.top}")
    else:
        for name, default in smoothing.DEFAULTS.items():
            if getattr(a, "smooth_" + name) != default:
                ap.error(f"--smooth-{'no-pairs' if name == 'pairs' else name.replace('_', '-')} needs --smooth")
    return a, ap


def main(argv=None, emit=print):
    a, ap = parse_args(argv)
    try:
        cal = Calibration.from_json(a.calib)
    except (OSError, ValueError) as e:
        ap.error(f"--calib {a.calib}: {e}")
    K.require_dir(ap, "depth", a.depth)
    K.require_gpu()
    reg = Registration(cal, a.scale, a.depth_unit, a.radial)
    os.makedirs(a.out, exist_ok=True)
    if a.temporal_filter is not None:
        files = filtering.stream_files(a.temporal_filter, ap, a.depth, a.depth_bits, a.top, a.depth_max, reg.device, a.stats)
    else:
        files = ((name, codes, None) for name, codes in K.depth_files(a.depth, a.depth_bits, a.top, reg.device))
    for name, codes, filtered in files:
        cleaned = None
        if a.cleaner is not None:
            codes = a.cleaner(codes, a.depth_max, stats=a.stats)
            codes, cleaned = codes if a.stats else (codes, None)
        smoothed = None
        if a.smoother is not None:
            codes = a.smoother(codes, a.depth_max, stats=a.stats)
            codes, smoothed = codes if a.stats else (codes, None)
        got = reg(codes, a.depth_max, stats=a.stats)
        out, counts = got if a.stats else (got, None)
        K.write_codes(os.path.join(a.out, name), out)
        if a.stats:
            c = counts.cpu().numpy().view(np.uint32)[0]
            tail = "" if filtered is None else " temporal: " + filtering.stats_line(filtered.cpu().numpy())
            tail += "" if cleaned is None else " cleaned: " + cleaning.stats_line(cleaned.cpu().numpy()[0])
            tail += "" if smoothed is None else " smoothed: " + smoothing.stats_line(smoothed.cpu().numpy()[0])
            emit(f"{name} " + " ".join(f"{k}={int(v)}" for k, v in zip(STATS, c)) + tail)
        else:
            emit(name)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
