"""Undistortion of the colour images: the step `codon_amd.register` asks for.  The colour camera's images, with
the Brown distortion of its lens, are resampled on the device to a pinhole camera, and the calibration is written again with
`color` replaced by that camera -- so `register --calib` accepts the copy and projects onto exactly the grid the images now have.

    python -m codon_amd.undistort --color DIR --calib FILE --out DIR [--calib-out FILE] [--focal-scale F] [--gray] [--stats]

A Catmull-Rom resampling in integers (tests/undistort_ref.py; csrc/undistort.hip): every target pixel's source position, through
the Brown model, in 1/32 source pixels; sixteen taps, weights in Q11, a border that repeats the edge; pixels whose source
position lies outside the image, or beyond the radius at which the radial model folds over, are black.  Only the tables are
floating point, float64 on the host, once.  Not handled: a fisheye or rational lens model, choosing the output camera
automatically (OpenCV's "optimal new camera matrix": --focal-scale is the user's), 16-bit guidance images, a rolling shutter."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os

import numpy as np
import torch

from . import _lib as L
from . import ops
from .codes import require_dir, require_gpu
from .register import MAX_SIDE, Camera, distort

OUTSIDE = -(1 << 20)
R2_MAX = 16.0
COUNTS = ("staged", "direct", "empty", "outside")


# ---- the tables: numpy on the host, float64, once (tests/undistort_ref.py restates them) ----------------------------------------------

def out_camera(src: Camera, focal_scale: float = 1.0) -> Camera:
    """The default output camera: src without its distortion, fx and fy multiplied by focal_scale (below 1: a wider view, which
    keeps the corners a barrel lens saw; above 1: a narrower one, which leaves no black border)"""
    try:
        f = float(focal_scale)
    except (TypeError, ValueError):
        f = float("nan")
    if not (f > 0.0 and math.isfinite(f)):
        raise ValueError(f"out_camera: focal_scale {focal_scale!r} (a positive number)")
    return Camera(src.width, src.height, src.fx * f, src.fy * f, src.cx, src.cy)


def r2_fold(dist) -> float:
    """The first rho on the grid n / 4096, n = 0 .. 65536, at which d(r radial(r^2)) / dr = 1 + 3 k1 rho + 5 k2 rho^2 + 7 k3 rho^3
    is not positive: where the radial model stops increasing (the tangential terms are ignored); inf without one"""
    k1, k2, _, _, k3 = dist
    rho = np.arange(65537, dtype=np.float64) / 4096.0
    at = np.flatnonzero(1.0 + 3.0 * k1 * rho + 5.0 * k2 * rho * rho + 7.0 * k3 * rho * rho * rho <= 0.0)
    return float(rho[at[0]]) if at.size else math.inf


def map_table(src: Camera, dst: Camera) -> np.ndarray:
    """M: int32 (dst.height, dst.width, 2), the source position of every target pixel in Q5 source pixels, (OUTSIDE, OUTSIDE)
    where it lies outside the source image, beyond r^2 = 16 or beyond the fold of the radial model"""
    if not isinstance(src, Camera) or not isinstance(dst, Camera):
        raise ValueError("map_table: src and dst must be Camera records")
    if any(dst.dist):
        raise ValueError(f"map_table: dst.dist {dst.dist!r} is not zero: the output camera is a pinhole camera")
    j, i = np.meshgrid(np.arange(dst.width, dtype=np.float64), np.arange(dst.height, dtype=np.float64))
    x, y = (j - dst.cx) / dst.fx, (i - dst.cy) / dst.fy
    xd, yd = distort(x, y, src.dist)
    with np.errstate(invalid="ignore", over="ignore"):
        U, V = np.rint(32.0 * (src.fx * xd + src.cx)), np.rint(32.0 * (src.fy * yd + src.cy))
        r2 = x * x + y * y
        out = ~np.isfinite(U) | ~np.isfinite(V) | (U < -16) | (U >= 32 * src.width - 16) | (V < -16) | (V >= 32 * src.height - 16)
        out |= (r2 > R2_MAX) | (r2 >= r2_fold(src.dist))
    return np.stack([np.where(out, OUTSIDE, U), np.where(out, OUTSIDE, V)], axis=-1).astype(np.int32)


def weight_table() -> np.ndarray:
    """K: int16 (32, 4), rint(2048 keys(p / 32)) at the taps -1, 0, 1, 2 (the Keys cubic with a = -0.5: Catmull-Rom), the first of
    the largest entries of a row adjusted so that every row sums to 2048"""
    t = np.abs(np.arange(32, dtype=np.float64)[:, None] / 32.0 - np.array([-1.0, 0.0, 1.0, 2.0])[None, :])
    k = np.where(t <= 1.0, (1.5 * t - 2.5) * t * t + 1.0, np.where(t < 2.0, ((-0.5 * t + 2.5) * t - 4.0) * t + 2.0, 0.0))
    K = np.rint(2048.0 * k).astype(np.int64)
    for row in K:
        row[int(np.argmax(row))] += 2048 - int(row.sum())
    return K.astype(np.int16)


def tile_table(src: Camera, M: np.ndarray):
    """(tiles int32 (ty, tx, 4), counts uint32[4]) of a map: the C entry codon_undistort_plan on the host, where the rule is"""
    lib = L.load()
    M = np.ascontiguousarray(M, dtype=np.int32)
    if M.ndim != 3 or M.shape[2] != 2:
        raise ValueError(f"tile_table: a map of shape {M.shape} ((ho, wo, 2))")
    ho, wo = M.shape[:2]
    nbytes = lib.codon_undistort_tiles_bytes(ho, wo)
    if nbytes == 0:
        raise ValueError(f"tile_table: a {ho}x{wo} target (1..{MAX_SIDE} each way)")
    tiles = np.zeros(nbytes // 4, dtype=np.int32)
    counts = np.zeros(4, dtype=np.uint32)
    P_ = C.c_void_p
    L.check(lib.codon_undistort_plan(src.height, src.width, ho, wo, P_(M.ctypes.data), P_(tiles.ctypes.data), P_(counts.ctypes.data)),
            "undistort_plan")
    return tiles.reshape(-(-ho // 8), -1, 4), counts


def rectified(mapping: dict, dst: Camera) -> dict:
    """The calibration mapping with `color` replaced by dst, a pinhole camera; every other key passes through untouched"""
    if not isinstance(mapping, dict):
        raise ValueError("rectified: the calibration must be a mapping")
    if not isinstance(dst, Camera) or any(dst.dist):
        raise ValueError("rectified: dst must be a Camera without distortion")
    out = dict(mapping)
    out["color"] = {"width": int(dst.width), "height": int(dst.height), "fx": dst.fx, "fy": dst.fy, "cx": dst.cx, "cy": dst.cy,
                    "dist": [0.0] * 5}
    return out


# ---- the device side ----------------------------------------------------------------------------------------------------------------

class Undistortion:
    """A colour camera's tables on the device.  und(img) resamples a batch of its images to the pinhole camera `.dst`;
    `.counts`: the plan's staged, direct and empty tiles and the outside pixels of one image."""

    def __init__(self, src: Camera, dst: Camera = None, focal_scale: float = 1.0, device=None):
        if not isinstance(src, Camera):
            raise ValueError("Undistortion: src must be a Camera")
        self.src = src
        self.dst = out_camera(src, focal_scale) if dst is None else dst
        M = map_table(src, self.dst)
        tiles, counts = tile_table(src, M)
        self.counts = {k: int(v) for k, v in zip(COUNTS, counts)}
        self.device = torch.device("cuda:0" if device is None else device)
        self.map = torch.from_numpy(M).to(self.device)
        self.tiles = torch.from_numpy(tiles).to(self.device)
        self.weights = torch.from_numpy(weight_table()).to(self.device)

    def __call__(self, img: torch.Tensor, channels: int = 1) -> torch.Tensor:
        """img: uint8 on this object's device, (H, W) or (B, H, W) grey, or with channels=3 (H, W, 3) or (B, H, W, 3) RGB, of the
        camera's size -> the same form at the output camera's size; the argument is not modified.  One launch."""
        who = "undistort"
        if channels not in (1, 3):
            raise ValueError(f"{who}: channels {channels!r} (1: grey, 3: RGB)")
        if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8:
            raise RuntimeError(f"{who} expects a uint8 tensor, got {getattr(img, 'dtype', type(img).__name__)}")
        if channels == 3 and (img.dim() not in (3, 4) or img.shape[-1] != 3):
            raise ValueError(f"{who}: a tensor of shape {tuple(img.shape)} with channels=3 ((H, W, 3) or (B, H, W, 3): the last "
                             "dimension is the colour)")
        if channels == 1 and img.dim() not in (2, 3):
            raise ValueError(f"{who}: a tensor of shape {tuple(img.shape)} with channels=1 ((H, W) or (B, H, W))")
        lead = img.shape[:-1] if channels == 3 else img.shape
        h, w = lead[-2:]
        if (h, w) != (self.src.height, self.src.width):
            raise ValueError(f"{who}: a {h}x{w} image, and the camera is {self.src.height}x{self.src.width}")
        src = img.contiguous()
        dev = ops._dev(src)
        if dev != self.map.device:
            raise RuntimeError(f"{who}: the image on {dev}, the tables on {self.map.device}")
        B = lead[0] if len(lead) == 3 else 1
        tail = (3,) if channels == 3 else ()
        out = torch.empty((*lead[:-2], self.dst.height, self.dst.width, *tail), dtype=torch.uint8, device=dev)
        P_ = C.c_void_p
        with torch.cuda.device(dev):
            L.check(L.load().codon_undistort(B, h, w, channels, P_(src.data_ptr()), self.dst.height, self.dst.width,
                                             P_(self.map.data_ptr()), P_(self.tiles.data_ptr()), P_(self.weights.data_ptr()),
                                             P_(out.data_ptr()), ops._stream(dev)), who)
        return out


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m codon_amd.undistort", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--color", required=True, metavar="DIR", help="the colour camera's images, as the sensor wrote them")
    ap.add_argument("--calib", required=True, metavar="FILE", help="the rig's JSON; only color (width, height, fx, fy, cx, cy, dist) "
                    "is read")
    ap.add_argument("--out", required=True, metavar="DIR", help="where the undistorted images go, under the same file names")
    ap.add_argument("--calib-out", default=None, metavar="FILE", help="the calibration with color replaced by the output camera: "
                    "what register --calib then reads")
    ap.add_argument("--focal-scale", type=float, default=1.0, metavar="F",
                    help="the output camera's fx, fy over the calibrated ones (default 1.0; below 1 keeps more of the field)")
    ap.add_argument("--gray", action="store_true", help="convert to grey first, as the guidance is read, and write grey")
    ap.add_argument("--stats", action="store_true", help="print outside=, staged=, direct= and empty= per file")
    a = ap.parse_args(argv)
    if not (a.focal_scale > 0.0 and math.isfinite(a.focal_scale)):
        ap.error(f"--focal-scale {a.focal_scale} must be positive and finite")
    if os.path.abspath(a.out) == os.path.abspath(a.color):
        ap.error("--out is --color: the undistorted images would overwrite the sensor's")
    return a, ap


def main(argv=None, emit=print):
    from PIL import Image
    a, ap = parse_args(argv)
    try:
        with open(a.calib) as fh:
            mapping = json.load(fh)
        if not isinstance(mapping, dict) or "color" not in mapping:
            raise ValueError("Calibration: missing color")
        src = Camera.from_mapping(mapping["color"], "color")
    except (OSError, ValueError) as e:                                   # json.JSONDecodeError is a ValueError
        ap.error(f"--calib {a.calib}: {e}")
    require_dir(ap, "color", a.color)
    require_gpu()
    und = Undistortion(src, focal_scale=a.focal_scale)
    os.makedirs(a.out, exist_ok=True)
    for name in sorted(os.listdir(a.color)):
        im = Image.open(os.path.join(a.color, name))
        gray = a.gray or im.mode == "L"
        pic = np.asarray(im.convert("L" if gray else "RGB"), dtype=np.uint8)
        if pic.shape[:2] != (src.height, src.width):
            raise SystemExit(f"{os.path.join(a.color, name)}: a {pic.shape[0]}x{pic.shape[1]} image, and the colour camera of the "
                             f"calibration is {src.height}x{src.width}")
        got = und(torch.from_numpy(pic.copy()).to(und.device), 1 if gray else 3).cpu().numpy()
        Image.fromarray(got, mode="L" if gray else "RGB").save(os.path.join(a.out, name))
        c = und.counts
        emit(f"{name} outside={c['outside']} staged={c['staged']} direct={c['direct']} empty={c['empty']}" if a.stats else name)
    if a.calib_out:
        with open(a.calib_out, "w") as fh:
            json.dump(rectified(mapping, und.dst), fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
