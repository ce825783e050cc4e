"""Either side of the network in the reference's script, on device:
  postprocess_u8  clip -> *255 -> truncating uint8          /root/reference/CODON_X4/test.py:127-132
  masked_rmse     RMSE over label != 0, exact integer sums   /root/reference/CODON_X4/test.py:148-164
  postprocess_u16, masked_rmse_u16   their 16-bit counterparts: definitions of this project, no reference
  depth_errors, depth_report   the evaluation suite: MAD, RMSE, max, bad-pixel rates, delta accuracies and the
                  edge / flat split from sixteen exact integer words per image, one launch; definitions of this project
  ssim            ssim_exact(img1, img2)                     /root/reference/CODON_X4/ssim_2.py:36-52
  L1SSIMLoss      w_l1 * mean|p - t| + w_ssim * (1 - SSIM(p, t)) with a HIP backward (the reference ships no
                  loss -- SURVEY D8 -- so the combination is this repo's; the SSIM value is pinned).
  MaskedL1SSIMLoss  the same loss over the valid pixels only (holes = target 0, masked_rmse's rule)."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from . import ops


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def postprocess_u8(x: torch.Tensor) -> torch.Tensor:
    """np.clip(out, 0, 1); (out * 255).astype(np.uint8) with the product formed in the array's dtype, as numpy
    does: an fp16 network output (the reference script's default) is rounded to fp16 before the truncating cast
    (test.py:125-132).  bf16 has no numpy counterpart: it is upcast to fp32.  This rule (truncation) is the reference's and is
    pinned to it; the 16-bit rule, postprocess_u16, rounds to nearest and is pinned to nothing."""
    lib = L.load()
    if x.dtype not in (torch.float32, torch.float16):
        x = x.float()
    x = x.contiguous()
    dev = ops._dev(x)
    out = torch.empty(x.shape, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.codon_postprocess_u8_dt(x.numel(), _p(x), ops._dt(x), _p(out), ops._stream(dev)), "postprocess_u8")
    return out


def _sqerr_dev(label: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """int64[2] = { sum of squared errors, count over label != 0 } on the device, for u8 planes or (after _as_u16) u16 codes;
    the label is cropped to the output's size."""
    lib = L.load()
    assert label.dtype == out.dtype and out.dtype in (torch.uint8, torch.uint16) and out.dim() == 2, (label.dtype, out.dtype)
    wide = out.dtype == torch.uint16
    if wide:
        label = label.view(torch.int16)              # slicing and .contiguous() where an op lacks uint16: the same bits
    label = label[:out.shape[0], :out.shape[1]].contiguous()
    out = out.contiguous()
    dev = ops._dev(label, out)
    acc = torch.empty(2, dtype=torch.int64, device=dev)
    fn, what = (lib.codon_masked_sqerr_u16, "masked_sqerr_u16") if wide else (lib.codon_masked_sqerr, "masked_sqerr")
    with torch.cuda.device(dev):
        L.check(fn(out.numel(), _p(label), _p(out), _p(acc), ops._stream(dev)), what)
    return acc


def _rmse(label: torch.Tensor, out: torch.Tensor) -> float:
    s, c = (int(v) for v in _sqerr_dev(label, out).cpu())
    return math.sqrt(s / c)


def masked_sqerr_dev(label_u8: torch.Tensor, out_u8: torch.Tensor) -> torch.Tensor:
    """masked_rmse's two exact integer sums as a DEVICE tensor int64[2] = { sum of squared errors, count } -- no host
    synchronisation (codon_amd.infer reads them back one image later); rmse = sqrt(s / c)."""
    assert label_u8.dtype == torch.uint8 and out_u8.dtype == torch.uint8
    return _sqerr_dev(label_u8, out_u8)


def masked_rmse(label_u8: torch.Tensor, out_u8: torch.Tensor) -> float:
    """test.py::EvaluationResults: label is cropped to the output's size (:151); pixels with label == 0 are
    excluded from both the error and the count."""
    assert label_u8.dtype == torch.uint8 and out_u8.dtype == torch.uint8
    return _rmse(label_u8, out_u8)


def _as_u16(t: torch.Tensor) -> torch.Tensor:
    """u16 codes are held as torch.uint16, or as an int16 view of the same bits where an op lacks uint16."""
    if t.dtype == torch.int16:
        return t.view(torch.uint16)
    assert t.dtype == torch.uint16, t.dtype
    return t


def codes_to_float(t_u16: torch.Tensor) -> torch.Tensor:
    """fp32 of u16 codes (exact), through int32: not every device op takes uint16."""
    return (_as_u16(t_u16).view(torch.int16).to(torch.int32) & 0xFFFF).float()


def postprocess_u16(x: torch.Tensor, depth_max: int = 65535) -> torch.Tensor:
    """code = rint(clamp(out, 0, 1) * float32(depth_max)) as torch.uint16: round half to even, the product formed in fp32
    (fp16 and bf16 outputs are upcast first, in the kernel), NaN -> 0.  UNPINNED by nature: the reference writes 8-bit images
    only (postprocess_u8 is its rule), so this is the project's definition, restated in tests/train_data16_ref.py."""
    lib = L.load()
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        x = x.float()
    x = x.contiguous()
    dev = ops._dev(x)
    out = torch.empty(x.shape, dtype=torch.uint16, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.codon_postprocess_u16_dt(x.numel(), _p(x), ops._dt(x), int(depth_max), _p(out), ops._stream(dev)),
                "postprocess_u16")
    return out


def masked_sqerr_u16_dev(label_u16: torch.Tensor, out_u16: torch.Tensor) -> torch.Tensor:
    """masked_sqerr_dev over u16 codes: a DEVICE tensor int64[2] = { sum of squared errors, count over label != 0 }."""
    return _sqerr_dev(_as_u16(label_u16), _as_u16(out_u16))


def masked_rmse_u16(label_u16: torch.Tensor, out_u16: torch.Tensor) -> float:
    """masked_rmse in 16-bit codes: label cropped to the output's size, label == 0 excluded."""
    return _rmse(_as_u16(label_u16), _as_u16(out_u16))


# ---- depth evaluation suite ---------------------------------------------------------------------------------------

EVAL_WORDS, EVAL_MAX_THRESHOLDS, EVAL_MAX_RADIUS = 16, 4, 8


def _label_and_output(who, label, out):
    """The dtype and shape rules of depth_errors' two planes -> (label, out) as (B, H, W), whether a single (H, W) plane came in,
    and the output's own dtype"""
    if label.dtype != out.dtype and {label.dtype, out.dtype} == {torch.int16, torch.uint16}:
        label = label.view(out.dtype)                 # the same bits
    if label.dtype != out.dtype or out.dtype not in (torch.uint8, torch.uint16, torch.int16):
        raise ValueError(f"{who}: label {label.dtype} and output {out.dtype} (both uint8, or both u16 codes as uint16 / int16)")
    if label.dim() != out.dim() or out.dim() not in (2, 3):
        raise ValueError(f"{who}: planes of shape {tuple(label.shape)} and {tuple(out.shape)} ((H, W) or (B, H, W))")
    single = out.dim() == 2
    if single:
        label, out = label[None], out[None]
    if label.shape[0] != out.shape[0]:
        raise ValueError(f"{who}: {label.shape[0]} labels for {out.shape[0]} outputs")
    return label, out, single, out.dtype


def _label_by_strides(label, out, wide):
    """The layout rules of depth_errors' two planes -> (label, read through its own strides; out, contiguous; their device)"""
    if wide:
        label, out = label.view(torch.int16), out.view(torch.int16)     # the same bits, in a dtype every device op takes
    Bl, Hl, Wl = label.shape
    if label.stride(2) != 1 or label.stride(1) < Wl or (Bl > 1 and label.stride(0) < label.stride(1) * (Hl - 1) + Wl):
        label = label.contiguous()                    # a layout the entry does not take (an expanded batch, a transposed plane)
    out = out.contiguous()
    dev = ops._dev(out)                               # the label goes by its strides: a window of a larger plane is welcome
    if label.device != dev:
        raise RuntimeError("codon_amd: tensors on different devices")
    return label, out, dev


def depth_errors(label: torch.Tensor, out: torch.Tensor, *, thresholds=(), edge_threshold=None, edge_radius=1,
                 error_map=False, region_map=False):
    """The evaluation words of (H, W) or (B, H, W) code planes in ONE launch (codon_depth_errors), no host synchronisation:
    a DEVICE int64 (B, 16) tensor per image -- 0 n, 1 sum e, 2 sum e^2, 3 max e, 4-7 #{e > thresholds[k]}, 8-10 the delta < 1.25 /
    1.25^2 / 1.25^3 inliers, 11-13 n, sum e, sum e^2 over the edge region, 14-15 zero -- over the pixels with label != 0,
    e = |label - out| in codes, exact integers (depth_report turns a row into MAD, RMSE, rates).  Both planes uint8, or both u16
    codes held as uint16 or int16 bits.  The label is at least as large as the output and is read top-left through its own
    strides (no cropped copy; only a layout whose rows or images overlap or whose pixels are not adjacent, such as a label
    expanded over the batch, is copied first).  thresholds: up to four integers >= 0, codes.  edge_threshold None: no edge evaluation; else
    the edge region is every valid pixel within Chebyshev distance edge_radius (0..8) of a valid pixel that has a valid
    4-neighbour differing by more than edge_threshold codes (the sensor model's edge rule).
    Returns the words alone, or (words, error map, region map) with the maps asked for: the error map has the codes' own dtype
    (e where valid, else 0), the region map is uint8 (0 hole, 1 valid and flat, 2 valid and in the edge region)."""
    lib = L.load()
    label, out, single, carrier = _label_and_output("depth_errors", label, out)
    thresholds = tuple(thresholds)
    if any(int(t) != t for t in thresholds) or (edge_threshold is not None and int(edge_threshold) != edge_threshold) \
            or int(edge_radius) != edge_radius:
        raise ValueError("depth_errors: thresholds, edge_threshold and edge_radius are integers (codes, pixels)")
    wide = carrier != torch.uint8
    label, out, dev = _label_by_strides(label, out, wide)
    B, H, W = out.shape
    d = L.DepthErrorsDesc(B, H, W, 16 if wide else 8, label.shape[1], label.shape[2], label.stride(1), label.stride(0),
                          len(thresholds), (C.c_int32 * 4)(*(int(t) for t in thresholds[:EVAL_MAX_THRESHOLDS])),
                          0 if edge_threshold is None else 1, 0 if edge_threshold is None else int(edge_threshold),
                          int(edge_radius))
    acc = torch.empty((B, EVAL_WORDS), dtype=torch.int64, device=dev)
    err = torch.empty_like(out) if error_map else None
    reg = torch.empty(out.shape, dtype=torch.uint8, device=dev) if region_map else None
    with torch.cuda.device(dev):
        L.check(lib.codon_depth_errors(C.byref(d), _p(label), _p(out), _p(acc), _p(err), _p(reg), ops._stream(dev)), "depth_errors")
    err = err.view(carrier) if err is not None else None
    maps = tuple(m[0] if single else m for m in (err, reg) if m is not None)
    return (acc, *maps) if maps else acc


def depth_report(acc_row, *, unit: float = 1.0, thresholds=()) -> dict:
    """One image's sixteen words (a row of depth_errors, on the host) as numbers, in Python floats: n; mad, rmse and max in
    codes times `unit`; "bad>t" for every threshold t (the fraction of valid pixels whose error exceeds t codes); delta1,
    delta2, delta3 (the fractions with max(l/o, o/l) < 1.25, 1.25^2, 1.25^3); edge_fraction = n_E / n; edge_mad, edge_rmse
    over the edge region and flat_mad, flat_rmse over the rest (words 0-2 minus words 11-13).  rmse is sqrt(word 2 / word 0):
    with unit 1 it equals masked_rmse / masked_rmse_u16 of the same planes to the bit.  A value over an empty set is nan (an
    image without a discontinuity is legitimate); n = 0 raises ZeroDivisionError, as the inference loop does."""
    w = [int(v) for v in acc_row]
    if len(w) != EVAL_WORDS:
        raise ValueError(f"depth_report: {len(w)} words (one row of depth_errors has {EVAL_WORDS})")
    thresholds = tuple(thresholds)
    if len(thresholds) > EVAL_MAX_THRESHOLDS:
        raise ValueError(f"depth_report: {len(thresholds)} thresholds (at most {EVAL_MAX_THRESHOLDS})")
    unit = float(unit)
    n, n_e = w[0], w[11]
    mean = lambda s, c: s / c if c else math.nan                                                       # noqa: E731
    r = {"n": n, "mad": w[1] / n * unit, "rmse": math.sqrt(w[2] / n) * unit, "max": w[3] * unit}
    for k, t in enumerate(thresholds):
        r[f"bad>{t}"] = w[4 + k] / n
    r.update(delta1=w[8] / n, delta2=w[9] / n, delta3=w[10] / n, edge_fraction=n_e / n,
             edge_mad=mean(w[12], n_e) * unit, edge_rmse=math.sqrt(mean(w[13], n_e)) * unit,
             flat_mad=mean(w[1] - w[12], n - n_e) * unit, flat_rmse=math.sqrt(mean(w[2] - w[13], n - n_e)) * unit)
    return r


def report_means(reports) -> dict:
    """Means of depth_report dicts over the images: {key: [mean over the images whose value is not nan, their count]}; the
    mean of no image is nan.  Every float-valued key: n and whatever the caller added (a file name) are left out."""
    out = {}
    for k in (k for k, v in (reports[0] if reports else {}).items() if isinstance(v, float)):
        vs = [r[k] for r in reports if not math.isnan(r[k])]
        out[k] = [sum(vs) / len(vs) if vs else math.nan, len(vs)]
    return out


def report_tokens(r: dict) -> str:
    """ key=value tokens of a depth_report dict, or of report_means (key=mean/count)."""
    return " ".join(f"{k}={v[0]!r}/{v[1]}" if isinstance(v, list) else f"{k}={v!r}" for k, v in r.items())


# ---- surface-normal angle error -------------------------------------------------------------------------------------

NORMAL_ANGLES, NORMAL_BINS, NORMAL_WORDS, NORMAL_MAX_THRESHOLDS, NORMAL_MAX_RADIUS = 1440, 1441, 1448, 4, 8
NORMAL_VALID, NORMAL_LABEL_NORMALS, NORMAL_COMPARED, NORMAL_OUT_HOLES = 1441, 1442, 1443, 1444
NORMAL_NONE = 65535                                   # the angle map's texel of a pixel that is not compared
NORMAL_DEFAULTS = dict(radius=2, tolerance=2, tolerance_rel=0.02)          # cloud's, untuned
NORMAL_THRESHOLDS = (11.25, 22.5, 30.0)


def angle_tables():
    """(C, S) int32 (1440 each): C[m - 1] = rint(2^30 cos t_m), S[m - 1] = rint(2^30 sin t_m) at the thresholds t_m = (m - 1/2) / 8
    degrees, m = 1 .. 1440, between the bins of an eighth of a degree; float64 on the host, once"""
    import numpy as np
    t = np.radians((np.arange(1, NORMAL_ANGLES + 1, dtype=np.float64) - 0.5) / 8.0)
    return np.rint(float(1 << 30) * np.cos(t)).astype(np.int32), np.rint(float(1 << 30) * np.sin(t)).astype(np.int32)


def _rays_of(who, camera, H, W):
    """(key, maker of (rx, ry) int32) of a register.Camera or of a pair of ray tables that cover an H x W window"""
    import numpy as np
    from .register import A_LIMIT, Camera
    if isinstance(camera, Camera):
        if any(camera.dist):
            raise ValueError(f"{who}: camera.dist {camera.dist!r} is not zero: a distorted camera has no separable ray table "
                             "(undistort the images first: python -m codon_amd.undistort --calib-out ...)")
        if camera.height < H or camera.width < W:
            raise ValueError(f"{who}: a {camera.height}x{camera.width} camera is smaller than the {H}x{W} output")
        from .cloud import ray_tables
        return ("camera", camera.width, camera.height, camera.fx, camera.fy, camera.cx, camera.cy), lambda: ray_tables(camera)
    try:
        rx, ry = (np.array(t.cpu() if isinstance(t, torch.Tensor) else t) for t in camera)      # copies: writable, contiguous
    except (TypeError, ValueError):
        raise ValueError(f"{who}: camera must be a register.Camera or a pair of int32 ray tables (RX, RY)") from None
    if rx.dtype != np.int32 or ry.dtype != np.int32 or rx.ndim != 1 or ry.ndim != 1:
        raise ValueError(f"{who}: camera must be a register.Camera or a pair of int32 ray tables (RX, RY)")
    if len(ry) < H or len(rx) < W:
        raise ValueError(f"{who}: ray tables of a {len(ry)}x{len(rx)} camera are smaller than the {H}x{W} output")
    if max(np.abs(rx[:W].astype(np.int64)).max(), np.abs(ry[:H].astype(np.int64)).max()) >= A_LIMIT:
        raise ValueError(f"{who}: a ray of 2^22 or more in Q20")
    return ("tables", rx.tobytes(), ry.tobytes()), lambda: (rx, ry)


_host_rays: dict = {}


def normal_errors(label: torch.Tensor, out: torch.Tensor, camera, *, radius=NORMAL_DEFAULTS["radius"],
                  tolerance=NORMAL_DEFAULTS["tolerance"], tolerance_rel=NORMAL_DEFAULTS["tolerance_rel"], depth_max=None,
                  angle_map=False):
    """The surface-normal angle error of (H, W) or (B, H, W) code planes in ONE launch (codon_normal_errors), no host
    synchronisation: a DEVICE int32 (B, 1448) tensor per image -- 0 .. 1440 the histogram of a = rint(8 angle in degrees) between
    the label's normal and the output's over the COMPARED pixels (label != 0 and both planes have a normal), 1441 the valid label
    pixels, 1442 those whose label has a normal, 1443 the compared pixels, 1444 the pixels with label != 0 and output == 0, 1445 ..
    1447 zero (normal_report turns a row into mean, median, RMSE and rates).  The normals are cloud's integer normals (radius,
    tolerance per step, tolerance_rel: its link parameters and its untuned defaults) and the output is masked by the label's
    holes first, so both see one hole set.  RIGHT ONLY WHERE CODE IS PROPORTIONAL TO METRIC z: true of every file this project
    reads, false of disparity files.  camera: the register.Camera of the label's grid (no distortion, at least as large as the
    output), or a pair (RX, RY) of int32 ray tables (cloud.ray_tables); a top-left crop keeps the principal point, so the first W
    and H entries are used.  Dtypes and layouts are depth_errors': uint8, or u16 codes as uint16 / int16; the label at least as
    large as the output, read top-left through its own strides.  depth_max: the largest code of a u16 set (default 65535);
    tolerance may not exceed it.  Returns the words alone, or (words, angle map) with angle_map: uint16, a where the pixel is
    compared, 65535 elsewhere."""
    from . import codes as K
    who = "normal_errors"
    lib = L.load()
    label, out, single, carrier = _label_and_output(who, label, out)
    wide = carrier != torch.uint8
    if not wide and depth_max not in (None, 255):
        raise ValueError(f"{who}: depth_max {depth_max!r} with 8-bit codes")
    top = 255 if not wide else 65535 if depth_max is None else K.integer(who, "depth_max", depth_max, 1, 65535, "1..65535")
    radius = K.integer(who, "radius", radius, 1, NORMAL_MAX_RADIUS, f"an integer in 1..{NORMAL_MAX_RADIUS}")
    tolerance = K.integer(who, "tolerance", tolerance, 0, top, f"an integer number of codes, 0 .. the largest code {top}")
    rel = K.rel_q16(who, tolerance_rel)
    B, H, W = out.shape
    if label.shape[1] < H or label.shape[2] < W:
        raise ValueError(f"{who}: a {label.shape[1]}x{label.shape[2]} label is smaller than the {H}x{W} output")
    key, make = _rays_of(who, camera, H, W)
    label, out, dev = _label_by_strides(label, out, wide)
    host = _host_rays.get(key)                        # the host's tables once per camera, their device copies once per device
    if host is None:
        host = _host_rays[key] = make()
    rx, ry = K.on_device(("normal_rx", key), lambda: host[0], dev), K.on_device(("normal_ry", key), lambda: host[1], dev)
    span = (C.c_int32 * 4)(int(host[0][0]), int(host[0][W - 1]), int(host[1][0]), int(host[1][H - 1]))
    ctab, stab = K.on_device("normal_cos", lambda: angle_tables()[0], dev), K.on_device("normal_sin", lambda: angle_tables()[1], dev)
    words = torch.empty((B, NORMAL_WORDS), dtype=torch.int32, device=dev)
    amap = torch.empty((B, H, W), dtype=torch.uint16, device=dev) if angle_map else None
    with torch.cuda.device(dev):
        L.check(lib.codon_normal_errors(B, H, W, _p(label), label.shape[1], label.shape[2], label.stride(1), label.stride(0), _p(out),
                                        L.FILL_U16 if wide else L.FILL_U8, top, _p(rx), _p(ry), span, _p(ctab), _p(stab), radius,
                                        tolerance, rel, _p(words), _p(amap), ops._stream(dev)), who)
    if amap is None:
        return words
    return words, (amap[0] if single else amap)


def normal_thresholds(thresholds, who="normal_report"):
    """The thresholds in degrees as a tuple of floats: at most four, each a multiple of 1/8 inside 0 .. 180; refusals by name"""
    thresholds = tuple(thresholds)
    if len(thresholds) > NORMAL_MAX_THRESHOLDS:
        raise ValueError(f"{who}: {len(thresholds)} thresholds (at most {NORMAL_MAX_THRESHOLDS})")
    for t in thresholds:
        ok = isinstance(t, (int, float)) and not isinstance(t, bool) and math.isfinite(t) and 0 <= t <= 180 and float(8 * t).is_integer()
        if not ok:
            raise ValueError(f"{who}: threshold {t!r} (degrees: a multiple of 1/8 in 0 .. 180)")
    return tuple(float(t) for t in thresholds)


def normal_report(row, thresholds=NORMAL_THRESHOLDS) -> dict:
    """One image's 1448 words (a row of normal_errors, on the host) as numbers, all in degrees, in Python floats: normal_n (the
    compared pixels), normal_coverage (compared / valid label pixels), normal_mean, normal_rmse, normal_median (the smallest a
    whose cumulative count reaches ceil(n / 2), over 8) and "normal<T" for every threshold T (the fraction of compared pixels with
    a <= 8 T).  A value over no compared pixel is nan, the report's rule, so report_means skips it."""
    w = [int(v) & 0xFFFFFFFF for v in row]
    if len(w) != NORMAL_WORDS:
        raise ValueError(f"normal_report: {len(w)} words (one row of normal_errors has {NORMAL_WORDS})")
    thresholds = normal_thresholds(thresholds)
    hist, n, valid = w[:NORMAL_BINS], w[NORMAL_COMPARED], w[NORMAL_VALID]
    if sum(hist) != n:
        raise ValueError(f"normal_report: the histogram holds {sum(hist)} pixels and word {NORMAL_COMPARED} says {n}")
    r = {"normal_n": n, "normal_coverage": n / valid if valid else math.nan}
    if n == 0:
        r.update(normal_mean=math.nan, normal_rmse=math.nan, normal_median=math.nan)
    else:
        half, run, median = (n + 1) // 2, 0, 0
        for a, v in enumerate(hist):
            run += v
            if run >= half:
                median = a
                break
        r.update(normal_mean=sum(a * v for a, v in enumerate(hist)) / (8 * n),
                 normal_rmse=math.sqrt(sum(a * a * v for a, v in enumerate(hist)) / n) / 8, normal_median=median / 8)
    for t in thresholds:
        r[f"normal<{t:g}"] = sum(hist[:int(8 * t) + 1]) / n if n else math.nan
    return r


def _ssim_forward(a, b, want_maps):
    lib = L.load()
    dev = ops._dev(a, b)
    assert a.shape == b.shape and a.dim() == 4 and a.shape[1] == 1 and a.dtype == torch.float32
    B, _, H, W = a.shape
    part = torch.empty(lib.codon_ssim_tiles(B, H, W), dtype=torch.float32, device=dev)
    dmaps = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if want_maps else None
    val = torch.empty(1, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.codon_ssim_fwd(B, H, W, _p(a), _p(b), _p(part), _p(dmaps), _p(val), ops._stream(dev)), "ssim_fwd")
    return val, dmaps


def ssim_dev(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """ssim() as a DEVICE tensor float64[1]: no host synchronisation."""
    if a.dim() == 2:
        a, b = a[None, None], b[None, None]
    v, _ = _ssim_forward(a.float().contiguous(), b.float().contiguous(), False)
    return v


def ssim(a: torch.Tensor, b: torch.Tensor) -> float:
    """mean SSIM of two (B,1,H,W) or (H,W) fp32 images in [0,1] (ssim_exact's definition)."""
    return float(ssim_dev(a, b).item())


def _bwd_buffers(p, dmaps):
    """Both backwards' buffers: (tmp, the row pass of the three derivative maps; ga, the gradient)."""
    return torch.empty_like(dmaps), torch.empty_like(p)


class _L1SSIMFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, w_l1, w_ssim):
        lib = L.load()
        p, t = pred.float().contiguous(), target.float().contiguous()
        dev = ops._dev(p, t)
        B, _, H, W = p.shape
        sval, dmaps = _ssim_forward(p, t, True)
        nparts = min(1024, (p.numel() + 255) // 256)
        part = torch.empty(nparts, dtype=torch.float32, device=dev)
        lval = torch.empty(1, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            L.check(lib.codon_l1_fwd(p.numel(), _p(p), _p(t), _p(part), nparts, _p(lval), ops._stream(dev)), "l1_fwd")
        ctx.save_for_backward(p, t, dmaps)
        ctx.w = (w_l1, w_ssim)
        return (w_l1 * lval + w_ssim * (1.0 - sval)).to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, g):
        p, t, dmaps = ctx.saved_tensors
        w_l1, w_ssim = ctx.w
        lib, dev, (B, _, H, W), n = L.load(), p.device, p.shape, p.numel()
        tmp, ga = _bwd_buffers(p, dmaps)
        # the kernel is linear in its two scales: run it for an upstream gradient of 1 and scale the 1-channel result by
        # g ON DEVICE -- float(g) here forced a host synchronisation in every training step
        with torch.cuda.device(dev):
            L.check(lib.codon_ssim_l1_bwd(B, H, W, _p(p), _p(t), _p(dmaps), _p(tmp), _p(ga),
                                          C.c_float(-w_ssim / n), C.c_float(w_l1 / n), ops._stream(dev)),
                    "ssim_l1_bwd")
        return ga.mul_(g.to(ga.dtype)), None, None, None


class L1SSIMLoss(torch.nn.Module):
    def __init__(self, w_l1: float = 1.0, w_ssim: float = 1.0):
        super().__init__()
        self.w_l1, self.w_ssim = w_l1, w_ssim

    def forward(self, pred, target):
        return _L1SSIMFn.apply(pred, target, self.w_l1, self.w_ssim)


# ---- hole-aware L1 + SSIM ---------------------------------------------------------------------------------------

def _valid_u8(valid, like):
    if valid is None:
        return None
    if valid.shape != like.shape:
        raise ValueError(f"valid mask of shape {tuple(valid.shape)} for images of shape {tuple(like.shape)}")
    if valid.dtype == torch.bool:
        valid = valid.to(torch.uint8)
    if valid.dtype != torch.uint8:
        raise ValueError(f"valid mask must be uint8 or bool (nonzero = valid), got {valid.dtype}")
    return valid.contiguous()


def _masked_forward(p, t, valid, w_l1, w_ssim, want_maps):
    """-> (value f64[1], counts i64 (B,2), per_image f64 (B,2), scales f32 (B,2), dmaps | None): two launches, no synchronisation."""
    lib = L.load()
    dev = ops._dev(p, t)
    assert p.shape == t.shape and p.dim() == 4 and p.shape[1] == 1 and p.dtype == t.dtype == torch.float32
    B, _, H, W = p.shape
    ws = torch.empty(4 * lib.codon_ssim_tiles(B, H, W), dtype=torch.float32, device=dev)
    dmaps = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if want_maps else None
    val = torch.empty(1, dtype=torch.float64, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
    per_image = torch.empty((B, 2), dtype=torch.float64, device=dev)
    scales = torch.empty((B, 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.codon_masked_l1_ssim_fwd(B, H, W, _p(p), _p(t), _p(valid), _p(ws), _p(dmaps), float(w_l1), float(w_ssim),
                                             _p(counts), _p(per_image), _p(scales), _p(val), ops._stream(dev)),
                "masked_l1_ssim_fwd")
    return val, counts, per_image, scales, dmaps


def masked_counts(target: torch.Tensor, valid: torch.Tensor = None) -> torch.Tensor:
    """(B,2) int64 on the device: {n_b, e_b} -- valid pixels of image b, and pixels whose whole 13x13 SSIM window is valid.
    valid: u8 / bool (B,1,H,W), nonzero = valid; None: target != 0."""
    t = target.float().contiguous()
    return _masked_forward(t, t, _valid_u8(valid, t), 1.0, 1.0, False)[1]


class _MaskedL1SSIMFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, valid, w_l1, w_ssim):
        p, t = pred.float().contiguous(), target.float().contiguous()
        v = _valid_u8(valid, t)
        val, _, _, scales, dmaps = _masked_forward(p, t, v, w_l1, w_ssim, ctx.needs_input_grad[0])
        if dmaps is not None:
            ctx.save_for_backward(p, t, dmaps, scales, *(() if v is None else (v,)))
        return val.to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, g):
        p, t, dmaps, scales, *v = ctx.saved_tensors
        v = v[0] if v else None
        lib, dev, (B, _, H, W) = L.load(), p.device, p.shape
        tmp, ga = _bwd_buffers(p, dmaps)
        up = g.to(torch.float32).reshape(1).contiguous()       # stays on the device: the kernel multiplies by it
        with torch.cuda.device(dev):
            L.check(lib.codon_masked_l1_ssim_bwd(B, H, W, _p(p), _p(t), _p(v), _p(dmaps), _p(scales), _p(up), _p(tmp), _p(ga),
                                                 ops._stream(dev)), "masked_l1_ssim_bwd")
        return ga, None, None, None, None


class MaskedL1SSIMLoss(torch.nn.Module):
    """(1/B) sum_b [ w_l1 * mean_valid |p - t| + w_ssim * (1 - mean_E ssim) ], the means per image: valid = the caller's mask or
    target != 0, E = the pixels whose whole SSIM window is valid.  Nothing stored at an invalid pixel of either image reaches
    the loss, and the gradient there is exactly +0."""

    def __init__(self, w_l1: float = 1.0, w_ssim: float = 1.0):
        super().__init__()
        self.w_l1, self.w_ssim = w_l1, w_ssim

    def forward(self, pred, target, valid=None):
        return _MaskedL1SSIMFn.apply(pred, target, valid, self.w_l1, self.w_ssim)
