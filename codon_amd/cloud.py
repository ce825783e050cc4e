"""Depth maps as coloured point clouds with normals: the way OUT of the pipeline.  Every non-zero code of a depth
map -- what `register`, `infer --lr-depth` or a label holds on the colour camera's grid, or a sensor's own z-depth file -- becomes
a point in metres (x right, y down, z forward) with a unit normal that faces the camera and, with --color, the pixel's colour, in
a binary little-endian PLY that a viewer opens.  The normal map (--normal-maps) is the picture depth super-resolution is judged by.

    python -m codon_amd.cloud --depth DIR --calib FILE --out DIR [--color DIR] [--camera {color,depth}] [--scale {1,4,8,16}]
                              [--depth-bits {8,16}] [--depth-max N] [--depth-unit M] [--no-normals] [--normal-radius R]
                              [--normal-tolerance CODES] [--normal-tolerance-rel F] [--normal-maps DIR] [--stats]
                              [--mesh [--mesh-tolerance CODES] [--mesh-tolerance-rel F]]

The definition (tests/cloud_ref.py; csrc/cloud.hip): the camera is two int32 ray tables in Q20, float64 on the host, once; a point
is code times ray in int64, one multiply in double and one conversion per component.  A normal is the cross product of two integer
tangents, each between the pixels --normal-radius steps away along an axis that are LINKED to the pixel (clean's rule, with
--normal-tolerance per step and --normal-tolerance-rel), one-sided where only one is; the pixels in between are not looked at.  A
pixel without a tangent on either axis has no normal (three zeros) and is still a point.  Records are packed on the device in
row-major order of the pixels -- count, scan, emit: three launches -- and the file's body is the device's bytes; the only host
synchronisation is the read of the counts, which sizes the download.  The four defaults (radius, tolerance, tolerance-rel, unit)
are untuned.  With --mesh the file is a triangle mesh over the same vertices (tests/mesh_ref.py; csrc/mesh_tile.h): a
pixel quad gives up to two triangles, each when its three corners are pairwise LINKED under --mesh-tolerance (one step, sides and
diagonals alike) and --mesh-tolerance-rel (both untuned); a quad of four takes the diagonal with the smaller code difference, a
quad of three has one candidate.  The 13-byte face records are packed on the device in row-major order of the quads -- six more
launches -- and the face count is read back with the point counts.  Not handled: in a mesh, hole filling, decimation, joining a
foreground to a background (unlinked corners give no triangle), and a retry of the other diagonal; a distorted camera (undistort
first); ranges along the ray (`register --radial` converts them); normals smoothed over more than two pixels per axis; any format
other than PLY.  (The normal-angle error between a label's normals and an output's is `infer --report --report-normals`, DESIGN
12.20: the same cd_normal.)"""
from __future__ import annotations

import argparse
import collections
import ctypes as C
import dataclasses
import os

import numpy as np
import torch

from . import _lib as L
from . import codes as K
from . import ops
from .codes import integer, rel_q16
from .register import A_LIMIT, SCALES, Calibration, Camera

MAX_RADIUS = 8
DEFAULTS = dict(depth_unit=0.001, radius=2, tolerance=2, tolerance_rel=0.02)
FRAME = "comment x right, y down, z forward, in metres"
STATS = ("points", "normals")
MESH_DEFAULTS = dict(tolerance=DEFAULTS["tolerance"], tolerance_rel=DEFAULTS["tolerance_rel"])       # cloud's link defaults: untuned
FACE_REC = 13                                  # the byte 3 and three int32 vertex indices
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])

# the packed body (B, h w rec) uint8 and counts (B, 2) int32 (points, points with a normal) on the device, the bytes of a record,
# the normal map (B, h, w, 3) uint8 or None
Cloud = collections.namedtuple("Cloud", "body counts rec normal_map")
# the packed face records (B, 2 (h - 1) (w - 1) 13) uint8 and counts (B) int32 (faces) on the device: image b's faces are
# body[b, :counts[b] * 13], their indices positions in the body of the same codes' Cloud
Faces = collections.namedtuple("Faces", "body counts")


def scaled_camera(cam: Camera, scale: int) -> Camera:
    """The camera of a map on `cam`'s grid over `scale`: fx / S, (cx + 0.5) / S - 0.5 -- projection_q8's rule"""
    if scale not in SCALES:
        raise ValueError(f"scaled_camera: scale {scale!r} (1, 4, 8 or 16)")
    if scale == 1:
        return cam
    if min(cam.height // scale, cam.width // scale) < 1:
        raise ValueError(f"scaled_camera: a {cam.height}x{cam.width} image leaves nothing at scale {scale}")
    s = float(scale)
    return dataclasses.replace(cam, width=cam.width // scale, height=cam.height // scale, fx=cam.fx / s, fy=cam.fy / s,
                               cx=(cam.cx + 0.5) / s - 0.5, cy=(cam.cy + 0.5) / s - 0.5)


def ray_tables(cam: Camera):
    """(RX int32 (width), RY int32 (height)): rint(2^20 (j - cx) / fx) and rint(2^20 (i - cy) / fy); a distorted camera and a
    ray of 2^22 or more in magnitude are refused by name"""
    if not isinstance(cam, Camera):
        raise ValueError("ray_tables: camera must be a register.Camera")
    if any(cam.dist):
        raise ValueError(f"ray_tables: dist {cam.dist!r} is not zero: a distorted camera has no separable ray table (undistort the "
                         "images first: python -m codon_amd.undistort --calib-out ...)")
    rx = np.rint(float(1 << 20) * (np.arange(cam.width, dtype=np.float64) - cam.cx) / cam.fx)
    ry = np.rint(float(1 << 20) * (np.arange(cam.height, dtype=np.float64) - cam.cy) / cam.fy)
    if max(np.abs(rx).max(), np.abs(ry).max()) >= A_LIMIT:
        raise ValueError("ray_tables: a ray of 2^22 or more in Q20 (|x_n| or |y_n| of 4 or more): the intrinsics do not describe "
                         "a camera this can unproject")
    return rx.astype(np.int32), ry.astype(np.int32)


def record_size(normals: bool, color: bool) -> int:
    return 12 + (12 if normals else 0) + (3 if color else 0)


def record_dtype(normals: bool, color: bool) -> np.dtype:
    f = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        f += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if color:
        f += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    return np.dtype(f)


def ply_header(count: int, normals: bool, color: bool, faces: int = None) -> bytes:
    """The fixed header of `count` packed records; faces: None, or the number of 13-byte face records behind them"""
    integer("ply_header", "count", count, 0, None, "an integer, 0 or more")
    if faces is not None:
        integer("ply_header", "faces", faces, 0, None, "None, or an integer, 0 or more")
    lines = ["ply", "format binary_little_endian 1.0", FRAME, f"element vertex {int(count)}"]
    lines += [f"property float {n}" for n in "xyz"]
    if normals:
        lines += [f"property float {n}" for n in ("nx", "ny", "nz")]
    if color:
        lines += [f"property uchar {n}" for n in ("red", "green", "blue")]
    if faces is not None:
        lines += [f"element face {int(faces)}", "property list uchar int vertex_indices"]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def write_ply(path: str, body, count: int, normals: bool, color: bool, faces=None, face_count: int = 0):
    """The header and the first count * rec bytes of `body` (bytes, or a uint8 array): nothing is interleaved here.  faces: None,
    or the face records (bytes, or a uint8 array): their first face_count * 13 bytes follow the vertices"""
    raw = body.tobytes() if isinstance(body, np.ndarray) else bytes(body)
    need = int(count) * record_size(normals, color)
    if len(raw) < need:
        raise ValueError(f"write_ply: {len(raw)} bytes of body, and {count} records take {need}")
    if faces is None:
        if face_count:
            raise ValueError(f"write_ply: face_count {face_count} without faces")
        with open(path, "wb") as fh:
            fh.write(ply_header(count, normals, color))
            fh.write(raw[:need])
        return
    tri = faces.tobytes() if isinstance(faces, np.ndarray) else bytes(faces)
    take = int(face_count) * FACE_REC
    if len(tri) < take:
        raise ValueError(f"write_ply: {len(tri)} bytes of faces, and {face_count} faces take {take}")
    with open(path, "wb") as fh:
        fh.write(ply_header(count, normals, color, int(face_count)))
        fh.write(raw[:need])
        fh.write(tri[:take])


def read_ply(path: str) -> np.ndarray:
    """A file `write_ply` wrote -> a structured array over its packed records (x, y, z[, nx, ny, nz][, red, green, blue]): a
    field is a view.  Anything else is refused by name"""
    with open(path, "rb") as fh:
        raw = fh.read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError(f"read_ply: {path} is not a PLY file")
    lines = raw[:end].decode("ascii", errors="replace").split("\n")
    try:
        count = int(next(ln for ln in lines if ln.startswith("element vertex ")).split()[2])
    except (StopIteration, ValueError):
        raise ValueError(f"read_ply: {path} names no vertex count") from None
    names = [ln.split()[-1] for ln in lines if ln.startswith("property ")]
    normals, color = "nx" in names, "red" in names
    body = raw[end + len(b"end_header\n"):]
    if raw[:end + len(b"end_header\n")] != ply_header(count, normals, color):
        raise ValueError(f"read_ply: {path}: not the header codon_amd.cloud writes")
    dt = record_dtype(normals, color)
    if len(body) != count * dt.itemsize:
        raise ValueError(f"read_ply: {path}: {len(body)} bytes of body, and {count} records take {count * dt.itemsize}")
    return np.frombuffer(body, dtype=dt)


def read_mesh(path: str):
    """A file `write_ply` wrote with faces -> (vertices: the structured array read_ply gives, faces: (F, 3) int32).  Anything
    else, a file without a face element included, is refused by name"""
    with open(path, "rb") as fh:
        raw = fh.read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError(f"read_mesh: {path} is not a PLY file")
    lines = raw[:end].decode("ascii", errors="replace").split("\n")
    try:
        count = int(next(ln for ln in lines if ln.startswith("element vertex ")).split()[2])
        tris = int(next(ln for ln in lines if ln.startswith("element face ")).split()[2])
    except (StopIteration, ValueError):
        raise ValueError(f"read_mesh: {path} names no vertex count or no face count") from None
    names = [ln.split()[-1] for ln in lines if ln.startswith("property ")]
    normals, color = "nx" in names, "red" in names
    body = raw[end + len(b"end_header\n"):]
    if raw[:end + len(b"end_header\n")] != ply_header(count, normals, color, tris):
        raise ValueError(f"read_mesh: {path}: not the header codon_amd.cloud writes")
    dt = record_dtype(normals, color)
    need = count * dt.itemsize + tris * FACE_REC
    if len(body) != need:
        raise ValueError(f"read_mesh: {path}: {len(body)} bytes of body, and {count} records with {tris} faces take {need}")
    rec = np.frombuffer(body, dtype=FACE_DTYPE, count=tris, offset=count * dt.itemsize)
    if not (rec["n"] == 3).all():
        raise ValueError(f"read_mesh: {path}: a face that is no triangle")
    return np.frombuffer(body, dtype=dt, count=count), np.ascontiguousarray(rec["v"])


def triangulate(codes: torch.Tensor, tolerance: int = MESH_DEFAULTS["tolerance"], tolerance_rel: float = MESH_DEFAULTS["tolerance_rel"],
                depth_max: int = None) -> Faces:
    """codes: (h, w) or (B, h, w) uint8 codes, or u16 codes as int16 / uint16, 0 a hole, on the device -> Faces: the triangles of
    the pixel quads whose corners are linked under tolerance (codes, for one step) and tolerance_rel, over the vertices
    Unprojection gives for the same codes.  Faces depend on the codes alone: no camera.  Six launches (one for a plane without a
    quad, which has no face); no host synchronisation."""
    who = "cloud_mesh"
    p = K.code_planes(who, codes, depth_max)
    B, h, w, top = p.B, p.h, p.w, p.top
    tol = integer(who, "tolerance", tolerance, 0, 65535, "an integer number of codes, 0 .. the largest code")
    rq = rel_q16(who, tolerance_rel)
    if tol > top:
        raise ValueError(f"{who}: tolerance {tol} above the largest code {top}")
    dev = p.dev
    body = torch.empty((B, 2 * (h - 1) * (w - 1) * FACE_REC), dtype=torch.uint8, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    P_ = C.c_void_p
    with ops._on(dev):
        ws = K.workspace(who, "codon_cloud_mesh_workspace_bytes", dev, B, h, w, batched=True)
        L.check(L.load().codon_cloud_mesh(B, h, w, p.ptr, p.fmt, top, tol, rq, P_(body.data_ptr()) if body.numel() else None,
                                          P_(counts.data_ptr()), P_(ws.data_ptr()), ws.numel(), ops._stream(dev)), who)
    return Faces(body, counts)


class Unprojection:
    """A camera's ray tables on the device.  un(codes) gives the packed records of a batch of planes of the camera's size.
    scale: the planes are on the camera's grid over `scale`; depth_unit: metres per code; radius, tolerance (codes per step),
    tolerance_rel: of the normals."""

    def __init__(self, camera: Camera, scale: int = 1, depth_unit: float = DEFAULTS["depth_unit"], normals: bool = True,
                 radius: int = DEFAULTS["radius"], tolerance: int = DEFAULTS["tolerance"],
                 tolerance_rel: float = DEFAULTS["tolerance_rel"], device=None):
        who = "Unprojection"
        if not isinstance(camera, Camera):
            raise ValueError(f"{who}: camera must be a register.Camera")
        if any(camera.dist):
            raise ValueError(f"{who}: camera.dist {camera.dist!r} is not zero: undistort the images first "
                             "(python -m codon_amd.undistort --calib-out ...)")
        if scale not in SCALES:
            raise ValueError(f"{who}: scale {scale!r} (1, 4, 8 or 16)")
        u = K.positive(who, "depth_unit", depth_unit, "a positive number of metres per code", allow_bool=False)
        self.camera = scaled_camera(camera, scale)
        self.scale, self.depth_unit, self.normals = scale, u, bool(normals)
        self.radius = integer(who, "radius", radius, 1, MAX_RADIUS, f"an integer in 1..{MAX_RADIUS}")
        self.tolerance = integer(who, "tolerance", tolerance, 0, 65535, "an integer number of codes, 0 .. the largest code")
        self.tolerance_rel = tolerance_rel
        self.tolerance_rel_q16 = rel_q16(who, tolerance_rel)
        self.m = u / float(1 << 20)
        rx, ry = ray_tables(self.camera)
        self.device = torch.device("cuda:0" if device is None else device)
        self.rx, self.ry = torch.from_numpy(rx).to(self.device), torch.from_numpy(ry).to(self.device)
        self._span = (C.c_int32 * 4)(int(rx[0]), int(rx[-1]), int(ry[0]), int(ry[-1]))

    def __call__(self, codes: torch.Tensor, color: torch.Tensor = None, depth_max: int = None, normal_map: bool = False) -> Cloud:
        """codes: (h, w) or (B, h, w) uint8 codes, or u16 codes as int16 / uint16, of the camera's size, 0 a hole, on this
        object's device; color: None, or uint8 (B, h, w) grey or (B, h, w, 3) RGB of the same planes (the batch axis as in
        codes) -> Cloud.  Image b's records are body[b, :counts[b, 0] * rec].  Three launches; no host synchronisation."""
        who = "cloud_points"
        p = K.code_planes(who, codes, depth_max)
        src, B, h, w, top = p.src, p.B, p.h, p.w, p.top
        cam = self.camera
        if (h, w) != (cam.height, cam.width):
            raise ValueError(f"{who}: a {h}x{w} plane, and the camera is {cam.height}x{cam.width}"
                             + (f" at scale {self.scale}" if self.scale != 1 else ""))
        if self.tolerance > top:
            raise ValueError(f"{who}: tolerance {self.tolerance} above the largest code {top}")
        if normal_map and not self.normals:
            raise ValueError(f"{who}: a normal map without normals")
        dev = p.dev
        if dev != self.rx.device:
            raise RuntimeError(f"{who}: codes on {dev}, the tables on {self.rx.device}")
        channels = 0
        if color is not None:
            lead = tuple(src.shape[:-2])
            if color.dtype != torch.uint8 or tuple(color.shape) not in (lead + (h, w), lead + (h, w, 3)):
                raise RuntimeError(f"{who} expects color as uint8 {lead + (h, w)} or {lead + (h, w, 3)}, not {color.dtype} "
                                   f"{tuple(color.shape)}")
            if color.device != dev:
                raise RuntimeError(f"{who}: codes on {dev}, color on {color.device}")
            channels = 3 if color.dim() == src.dim() + 1 else 1
            color = color.contiguous()
        rec = record_size(self.normals, channels != 0)
        body = torch.empty((B, h * w * rec), dtype=torch.uint8, device=dev)
        counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
        nmap = torch.empty((B, h, w, 3), dtype=torch.uint8, device=dev) if normal_map else None
        P_ = C.c_void_p
        with ops._on(dev):
            ws = K.workspace(who, "codon_cloud_workspace_bytes", dev, B, h, w, batched=True)
            L.check(L.load().codon_cloud_points(B, h, w, p.ptr, p.fmt, top,
                                                P_(self.rx.data_ptr()), P_(self.ry.data_ptr()), self._span, self.m, int(self.normals),
                                                self.radius, self.tolerance, self.tolerance_rel_q16,
                                                P_(color.data_ptr()) if channels else None, channels, P_(body.data_ptr()),
                                                P_(counts.data_ptr()), P_(nmap.data_ptr()) if normal_map else None,
                                                P_(ws.data_ptr()), ws.numel(), ops._stream(dev)), who)
        return Cloud(body, counts, rec, nmap)


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m codon_amd.cloud", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", required=True, metavar="DIR", help="depth maps: PNGs of codes, 0 a hole")
    ap.add_argument("--calib", required=True, metavar="FILE", help="the rig's calibration, as python -m codon_amd.register reads it")
    ap.add_argument("--out", required=True, metavar="DIR", help="where NAME.ply goes for every NAME.png")
    ap.add_argument("--color", default=None, metavar="DIR", help="8-bit grey or RGB images under the same file names, cropped "
                    "top-left to the depth map's size")
    ap.add_argument("--camera", default="color", choices=("color", "depth"),
                    help="color: a map register, infer or a label is on (default); depth: a sensor's own z-depth file")
    ap.add_argument("--scale", type=int, default=1, choices=SCALES, help="the maps are on the camera's grid over S (register --scale S)")
    K.add_depth_args(ap, depth_unit=DEFAULTS["depth_unit"])
    ap.add_argument("--no-normals", action="store_true", help="positions (and colours) alone")
    ap.add_argument("--normal-radius", type=int, default=DEFAULTS["radius"], metavar="R",
                    help="a tangent spans the pixels R steps away, 1..8 (default 2, untuned)")
    ap.add_argument("--normal-tolerance", type=int, default=DEFAULTS["tolerance"], metavar="CODES",
                    help="a far pixel counts when its code differs by at most R times this ... (default 2, untuned)")
    ap.add_argument("--normal-tolerance-rel", type=float, default=DEFAULTS["tolerance_rel"], metavar="F",
                    help="... plus this fraction of the smaller code (default 0.02, untuned)")
    ap.add_argument("--normal-maps", default=None, metavar="DIR", help="write the normals as RGB PNGs under the files' own names")
    ap.add_argument("--stats", action="store_true", help="print points= and normals= per file (and faces= with --mesh)")
    ap.add_argument("--mesh", action="store_true", help="write triangles too: NAME.ply is a mesh over the same vertices")
    ap.add_argument("--mesh-tolerance", type=int, default=None, metavar="CODES",
                    help=f"the corners of a triangle differ by at most this ... (default {MESH_DEFAULTS['tolerance']}, untuned)")
    ap.add_argument("--mesh-tolerance-rel", type=float, default=None, metavar="F",
                    help=f"... plus this fraction of the smaller code (default {MESH_DEFAULTS['tolerance_rel']}, untuned)")
    a = ap.parse_args(argv)
    a.top = K.depth_args_of(ap, a)
    if a.color is not None and a.scale != 1:
        ap.error(f"--color with --scale {a.scale}: the colour images are on the full grid; unproject a map at scale 1")
    if a.no_normals:
        if a.normal_maps is not None:
            ap.error("--normal-maps needs normals: drop --no-normals")
        for name in ("radius", "tolerance", "tolerance_rel"):
            if getattr(a, "normal_" + name) != DEFAULTS[name]:
                ap.error(f"--normal-{name.replace('_', '-')} with --no-normals")
    if not 1 <= a.normal_radius <= MAX_RADIUS:
        ap.error(f"--normal-radius {a.normal_radius} must be in [1, {MAX_RADIUS}]")
    if not 0 <= a.normal_tolerance <= a.top:
        ap.error(f"--normal-tolerance {a.normal_tolerance} must be in [0, {a.top}], the largest code")
    try:
        rel_q16("cloud", a.normal_tolerance_rel)
    except ValueError:
        ap.error(f"--normal-tolerance-rel {a.normal_tolerance_rel} must be in [0, 1)")
    for name in ("tolerance", "tolerance_rel"):
        if getattr(a, "mesh_" + name) is None:
            setattr(a, "mesh_" + name, MESH_DEFAULTS[name])
        elif not a.mesh:
            ap.error(f"--mesh-{name.replace('_', '-')} without --mesh")
    if not 0 <= a.mesh_tolerance <= a.top:
        ap.error(f"--mesh-tolerance {a.mesh_tolerance} must be in [0, {a.top}], the largest code")
    try:
        rel_q16("cloud", a.mesh_tolerance_rel)
    except ValueError:
        ap.error(f"--mesh-tolerance-rel {a.mesh_tolerance_rel} must be in [0, 1)")
    for other in ("depth", "color"):
        d = getattr(a, other)
        if d is not None and os.path.abspath(a.out) == os.path.abspath(d):
            ap.error(f"--out is --{other}")
    if a.normal_maps is not None and os.path.abspath(a.normal_maps) in {os.path.abspath(d) for d in (a.depth, a.color) if d}:
        ap.error("--normal-maps is --depth or --color: the maps would overwrite the inputs")
    return a, ap


def _read_color(path: str, h: int, w: int) -> np.ndarray:
    """An 8-bit grey (h, w) or RGB (h, w, 3) image, cropped top-left; a smaller one is refused by name"""
    from PIL import Image
    im = Image.open(path)
    if im.mode not in ("L", "RGB"):
        im = im.convert("RGB")
    a = np.asarray(im, dtype=np.uint8)
    if a.shape[0] < h or a.shape[1] < w:
        raise ValueError(f"{path}: {a.shape[0]}x{a.shape[1]}, smaller than the {h}x{w} of the depth map")
    return a[:h, :w].copy()


def main(argv=None, emit=print):
    a, ap = parse_args(argv)
    try:
        cal = Calibration.from_json(a.calib)
    except (OSError, ValueError) as e:
        ap.error(f"--calib {a.calib}: {e}")
    K.require_dir(ap, "depth", a.depth)
    if a.color is not None:
        K.require_dir(ap, "color", a.color)
    cam = cal.color if a.camera == "color" else cal.depth
    if any(cam.dist):
        hint = (": undistort the colour images first (python -m codon_amd.undistort --calib-out ...)" if a.camera == "color"
                else ": register the maps to the colour camera first (python -m codon_amd.register)")
        ap.error(f"--calib {a.calib}: {a.camera}.dist {cam.dist!r} is not zero{hint}")
    K.require_gpu()
    try:
        un = Unprojection(cam, a.scale, a.depth_unit, not a.no_normals, a.normal_radius, a.normal_tolerance, a.normal_tolerance_rel)
    except ValueError as e:
        ap.error(str(e))
    for d in (a.out, a.normal_maps):
        if d is not None:
            os.makedirs(d, exist_ok=True)
    for name, codes in K.depth_files(a.depth, a.depth_bits, a.top, un.device):
        color = None
        if a.color is not None:
            path = os.path.join(a.color, name)
            if not os.path.exists(path):
                raise ValueError(f"{path}: no colour image for {os.path.join(a.depth, name)}")
            color = torch.from_numpy(_read_color(path, *codes.shape)).to(un.device)
        got = un(codes, color, a.depth_max, normal_map=a.normal_maps is not None)
        tri = triangulate(codes, a.mesh_tolerance, a.mesh_tolerance_rel, a.depth_max) if a.mesh else None
        words = got.counts.reshape(-1) if tri is None else torch.cat([got.counts.reshape(-1), tri.counts])
        points, normals, *faces = (int(v) for v in words.cpu().numpy().view(np.uint32))     # the one host synchronisation
        body = got.body[0, :points * got.rec].cpu().numpy()
        path, line = os.path.join(a.out, os.path.splitext(name)[0] + ".ply"), f"{name} points={points} normals={normals}"
        if tri is None:
            write_ply(path, body, points, un.normals, color is not None)
        else:
            write_ply(path, body, points, un.normals, color is not None, tri.body[0, :faces[0] * FACE_REC].cpu().numpy(), faces[0])
            line += f" faces={faces[0]}"
        if a.normal_maps is not None:
            from PIL import Image
            Image.fromarray(got.normal_map[0].cpu().numpy(), mode="RGB").save(os.path.join(a.normal_maps, name))
        emit(line if a.stats else name)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
