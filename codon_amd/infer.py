"""python -m codon_amd.infer -- the reference's test loop (CODON_X4/test.py:60-145) on MI355X:
for every image: read depth (already HR-sized) + guidance, forward, clip/*255/uint8, write PNG, masked RMSE
vs the label, SSIM vs the label; print per-image values and the means.  Everything numeric runs in HIP kernels
(codon_amd.CODONNet, codon_amd.metrics); this file is I/O glue.

What is done with one image is written ONCE (_Plan: load -> enqueue -> settle, write) and the loop has two shapes.  One forward
of a Middlebury image takes 2.3 ms; decoding its two PNGs, the float conversion, the upload, the download and the PNG encode take
several times that on the host, and the reference's loop (test.py:109-145) does all of it serially per image.  By default the
steps sit on codon_amd.pipeline.run_pipeline, a torch-free skeleton with CPU tests of its own:
  reader threads: decode image i+1 (PIL releases the GIL), /255, cast, pinned host tensors, upload on a SIDE stream
  main thread   : launches and downloads of image i on the caller's stream (waits for the upload's event), then the host
                  arithmetic of image i-1, whose numbers have landed meanwhile
  writer thread : download of image i-1 has landed in pinned memory (event) -> PNG encode + write
A stage that fails -- the writer on a full disk, say -- raises in the caller; nothing hangs.  `--serial` is the same steps in turn
on the calling thread, uploads synchronous, no threads, no side stream: byte-identical outputs and lines by construction.

--lr-depth DIR instead of --input-depth: the depth files are LOW-RESOLUTION maps as a sensor writes them, code 0 a
hole.  The reader uploads the codes and the main stream turns them into the network's input with one launch
(codes_to_input: the training degradation's own hole-aware bicubic x--scale, back onto the code grid, cast), then the forward."""
from __future__ import annotations

import argparse
import math
import os
import time
from collections import namedtuple

import numpy as np
import torch

from . import CODONNet, CODONNet16, io, metrics
from .codes import codes_tensor
from .io import check_depth_max, list_pairs, read_depth_plane
from .pipeline import run_pipeline
from .prep import LrPrep, add_prep_args, prep_of
from .upsample import (FILL_SIGMA, JBU_SIGMA_S, bicubic_upsample_codes, check_fill_sigma, check_jbu_sigma_s, codes_to_input,
                       joint_bilateral_upsample, unstretch_codes)

BASELINES = ("bicubic", "jbu")


def _load_host(a_depth, a_color, a_label, f, tdt, depth_bits=8, depth_max=65535):
    """Host side of one image: decode, grey, /255 (float64 divide, then float32: test.py:116-123), crop both to the common
    size, cast to the model's dtype (the rounding `.cuda().half()` does on the device, done here on half the bytes).
    depth_bits=16: depth and label are 16-bit codes (io.read_depth_plane: an 8-bit file or a code above
    depth_max is refused), the depth input is float32(float64(c) / depth_max) before the same cast, the label is returned as
    an int16 view of its u16 bits; the guidance stays 8-bit.  depth_bits=8 refuses a 16-bit depth or label file."""
    # numpy only (single-threaded): torch's CPU ops fan a 170 k-element conversion out over every host core, which costs
    # milliseconds per call on a 128-core box; the values are io.to_input()'s -- float64 divide, float32, then the dtype's
    # round-to-nearest-even -- bit for bit
    px = read_depth_plane(os.path.join(a_depth, f), depth_bits, depth_max)
    py = io.read_gray(os.path.join(a_color, f))
    h, w = min(px.shape[0], py.shape[0]), min(px.shape[1], py.shape[1])
    lab = None
    if a_label:
        lab = codes_tensor(read_depth_plane(os.path.join(a_label, f), depth_bits, depth_max))
    return _plane(px[:h, :w], depth_max if depth_bits == 16 else 255, tdt), _plane(py[:h, :w], 255, tdt), lab, h, w


def _plane(p_, top, tdt):
    """(1,1,h,w) host tensor of dtype tdt: codes / top in float64, float32, then the dtype's round-to-nearest-even."""
    ndt = {torch.float32: np.float32, torch.float16: np.float16}.get(tdt)
    v = (np.asarray(p_) / top).astype(np.float32)
    if ndt is not None:
        return torch.from_numpy(np.ascontiguousarray(v.astype(ndt)))[None, None]
    # bf16 has no numpy type: round to nearest even on the bit pattern (finite, non-negative inputs)
    u = np.ascontiguousarray(v).view(np.uint32)
    b16 = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return torch.from_numpy(b16.view(np.int16)).view(torch.bfloat16)[None, None]


def _load_lr(a_lr, a_color, a_label, f, tdt, scale, depth_bits=8, depth_max=65535, with_guide=False):
    """Host side of one image under --lr-depth: the depth file is a LOW-RESOLUTION map of codes (0 a hole), read
    through io.read_depth_plane and returned AS CODES -- (h,w) uint8, or the u16 bits as int16 -- for codes_to_input; the
    HR size is (h * scale, w * scale), and the guidance and the label are cropped top-left to it.  A smaller guidance or label
    raises ValueError naming the file.  -> (codes, guidance, label or None, h, w) and a sixth, always there: with_guide
     the cropped guidance AS CODES, (H, W) uint8, for the guided hole filler, else None."""
    px = read_depth_plane(os.path.join(a_lr, f), depth_bits, depth_max)
    py = io.read_gray(os.path.join(a_color, f))
    h, w = px.shape[0] * scale, px.shape[1] * scale
    if py.shape[0] < h or py.shape[1] < w:
        raise ValueError(f"{os.path.join(a_color, f)}: {py.shape[0]}x{py.shape[1]}, smaller than the {h}x{w} that "
                         f"{os.path.join(a_lr, f)} gives at x{scale}")
    lab = None
    if a_label:
        lab = read_depth_plane(os.path.join(a_label, f), depth_bits, depth_max)
        if lab.shape[0] < h or lab.shape[1] < w:
            raise ValueError(f"{os.path.join(a_label, f)}: {lab.shape[0]}x{lab.shape[1]}, smaller than the {h}x{w} that "
                             f"{os.path.join(a_lr, f)} gives at x{scale}")
        lab = codes_tensor(lab[:h, :w])
    guide = torch.from_numpy(np.array(py[:h, :w])) if with_guide else None
    return codes_tensor(px), _plane(py[:h, :w], 255, tdt), lab, h, w, guide


READERS = int(os.environ.get("CODON_INFER_READERS", "3"))


def _pinned_copy(t: torch.Tensor) -> torch.Tensor:
    """t in page-locked memory, filled by a numpy copy: Tensor.pin_memory() copies with an at::parallel_for, i.e. spins up an
    OpenMP team of every host core in whichever thread calls it first (measured on the 128-core GPU box: 130 ms per image in a
    fresh reader thread)."""
    hp = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    if t.dtype == torch.bfloat16:
        hp.view(torch.int16).numpy()[...] = t.view(torch.int16).numpy()
    else:
        hp.numpy()[...] = t.numpy()
    return hp


# What the depth format (depth_bits, depth_max, depth_unit) decides, chosen once: post_codes(the network's map) -> codes;
# sqerr: (label, codes) -> int64[2] on the device; write(path, numpy codes); unit(codes) -> fp32 in [0, 1], what SSIM compares; the
# printed RMSE and the report are in codes times rmse_scale; depth_max as the upsample functions take it (None for 8-bit)
_Format = namedtuple("_Format", "post_codes sqerr write unit rmse_scale depth_max")


def _format(depth_bits, depth_max, depth_unit):
    if depth_bits == 16:
        top = float(depth_max)
        return _Format(lambda o: metrics.postprocess_u16(o, depth_max), metrics.masked_sqerr_u16_dev, io.write_depth16,
                       lambda t: metrics.codes_to_float(t) / top, float(depth_unit), depth_max)
    return _Format(metrics.postprocess_u8, metrics.masked_sqerr_dev, io.write_gray, lambda t: t.float() / 255, 1.0, None)


def _checked(model, input_depth, input_color, label, files, depth_bits, depth_max, lr_depth, scale, self_ensemble, report,
             fill_holes, normalize, fill_guided, fill_sigma, baseline, jbu_sigma_s, jbu_sigma_r):
    """Every refusal of run_loop, in their order of precedence -> (the preparation's record, the two checked jbu sigmas, the
    files: listed here, between the checks, where a missing directory has always been reported)."""
    if (lr_depth is None) == (input_depth is None):
        raise ValueError("run_loop: exactly one of input_depth and lr_depth")
    if depth_bits not in (8, 16):
        raise ValueError(f"run_loop: depth_bits {depth_bits!r} (8 or 16)")
    if depth_bits == 16:
        check_depth_max(depth_max)
    prep = LrPrep.checked("run_loop", fill_holes, fill_guided, fill_sigma, normalize, lr=("lr_depth", lr_depth is not None),
                          top=depth_max if depth_bits == 16 else 255)
    if baseline is not None:
        if baseline not in BASELINES:
            raise ValueError(f"run_loop: baseline {baseline!r} ({' or '.join(BASELINES)})")
        if lr_depth is None:
            raise ValueError("run_loop: baseline needs lr_depth (a baseline upsamples low-resolution code planes)")
        if self_ensemble:
            raise ValueError("run_loop: baseline with self_ensemble (there is no network to ensemble)")
        if baseline == "jbu":
            jbu_sigma_s, jbu_sigma_r = check_jbu_sigma_s("run_loop", jbu_sigma_s), check_fill_sigma("run_loop", jbu_sigma_r)
    if lr_depth is not None and scale not in (4, 8, 16):
        raise ValueError(f"run_loop: lr_depth needs scale 4, 8 or 16 (got {scale!r})")
    if model is None and baseline is None:
        raise ValueError("run_loop: model is None without a baseline")
    files = list_pairs(lr_depth or input_depth, input_color) if files is None else files
    if report is not None and not label:
        raise ValueError("run_loop: report needs label")
    return prep, jbu_sigma_s, jbu_sigma_r, files


# One image whose launches are enqueued: its name, the event recorded behind its downloads, and the pinned host buffers they land
# in -- the output codes, int64[2] squared error and count, float64[1] SSIM, the report's words, the error map, the normal report's
# words and its angle map; None where there is none
Pending = namedtuple("Pending", "f event codes acc ss words emap nwords nmap", defaults=(None, None))


def _write_angle_map(path, a):
    """An angle map of metrics.normal_errors as an 8-bit PNG: min(254, a // 8) degrees, 255 where the pixel is not compared"""
    a = np.asarray(a)
    io.write_gray(path, np.where(a == metrics.NORMAL_NONE, 255, np.minimum(254, a // 8)).astype(np.uint8))


def _download(t: torch.Tensor) -> torch.Tensor:
    """A pinned host buffer that t is being copied into behind the launches enqueued so far."""
    hp = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    hp.copy_(t, non_blocking=True)
    return hp


class _Plan:
    """What is done with one image, each step written once: load -> enqueue -> settle, write.  The serial loop calls them in turn
    on the calling thread; the pipelined loop hands the same four to pipeline.run_pipeline."""

    def __init__(self, dev, fmt, load_host, codes_of, out_dir, emit, report):
        """load_host(f) -> (x or codes, y, label or None, h, w, guidance codes or None) on the host; codes_of(x or codes, y,
        guidance codes) -> the output codes on the device; report: run_loop's, or None."""
        self.dev, self.fmt, self.load_host, self.codes_of, self.out_dir, self.emit = dev, fmt, load_host, codes_of, out_dir, emit
        self.stream = torch.cuda.current_stream(dev)
        self.rp_kw = self.err_dir = self.nm_kw = self.nm_dir = None
        if report is not None:
            self.rp_kw = {"thresholds": tuple(report.get("thresholds", ())), "edge_threshold": report.get("edge_threshold"),
                          "edge_radius": report.get("edge_radius", 1)}
            self.err_dir = report.get("error_maps")
            nm = report.get("normals")
            if nm is not None:                              # the normal report: one more launch behind depth_errors
                self.nm_kw = {"camera": nm["camera"], "depth_max": fmt.depth_max,
                              **{k: nm[k] for k in ("radius", "tolerance", "tolerance_rel") if k in nm}}
                self.nm_thresholds = metrics.normal_thresholds(nm.get("thresholds", metrics.NORMAL_THRESHOLDS), "run_loop")
                self.nm_dir = nm.get("error_maps")
        self.reports = []
        self.rm_sum = self.ss_sum = 0.0
        self.n = 0

    def load(self, f, up_s=None):
        """Image f on the device -> (f, [x or codes, y, label or None, guidance codes or None], the upload's event, h, w, the
        pinned sources).  up_s None: synchronous uploads on the current stream.  Else, for a reader thread: pinned buffers
        filled by numpy, uploads on the side stream up_s with an event behind them; the pinned sources ride along until the
        item is consumed."""
        x, y, lab, h, w, g = self.load_host(f)
        host = [x, y, lab, g]
        if up_s is None:
            return f, [t.to(self.dev) if t is not None else None for t in host], None, h, w, None
        torch.cuda.set_device(self.dev)
        host = [_pinned_copy(t) if t is not None else None for t in host]
        with torch.cuda.stream(up_s):
            devs = [t.to(self.dev, non_blocking=True) if t is not None else None for t in host]
            ev = torch.cuda.Event()
            ev.record(up_s)
        return f, devs, ev, h, w, host

    def enqueue(self, loaded):
        """Every launch of one image, in order -- [preparation ->] forward -> post-processing -> squared error -> SSIM -> report
        -- the downloads of what they give behind them, and one event behind those.  No host synchronisation."""
        f, (x, y, lab, g), ev, h, w, _host = loaded
        if ev is not None:
            self.stream.wait_event(ev)
            for t in (x, y, lab, g):
                if t is not None:
                    t.record_stream(self.stream)            # allocated on the upload stream, consumed on this one
        fmt = self.fmt
        codes = self.codes_of(x, y, g)
        acc = ss = words = emap = nwords = nmap = None
        if lab is not None:                                 # metrics stay on the device until settle()
            acc = fmt.sqerr(lab, codes)
            ss = metrics.ssim_dev(fmt.unit(lab[:h, :w]), fmt.unit(codes))
            acc, ss = _download(acc), _download(ss)
            if self.rp_kw is not None:                      # sixteen more words (and the error map) behind the same kernels
                r_ = metrics.depth_errors(lab, codes, error_map=bool(self.err_dir), **self.rp_kw)
                words = _download(r_[0][0] if self.err_dir else r_[0])
                emap = _download(r_[1]) if self.err_dir else None
                if self.nm_kw is not None:
                    n_ = metrics.normal_errors(lab, codes, angle_map=bool(self.nm_dir), **self.nm_kw)
                    nwords = _download(n_[0][0] if self.nm_dir else n_[0])
                    nmap = _download(n_[1]) if self.nm_dir else None
        codes = _download(codes)
        event = torch.cuda.Event()
        event.record(self.stream)
        return Pending(f, event, codes, acc, ss, words, emap, nwords, nmap)

    def settle(self, p):
        """The host arithmetic of an enqueued image (metrics.masked_rmse's and metrics.ssim's), its line and its report."""
        line = p.f
        if p.acc is not None:
            p.event.synchronize()
            s_, c_ = (int(v) for v in p.acc)
            rm, ss = math.sqrt(s_ / c_) * self.fmt.rmse_scale, float(p.ss.item())
            self.rm_sum += rm
            self.ss_sum += ss
            line += f" {rm} {ss}"
            if p.words is not None:
                rep = metrics.depth_report(p.words, unit=self.fmt.rmse_scale, thresholds=self.rp_kw["thresholds"])
                if p.nwords is not None:
                    rep.update(metrics.normal_report(p.nwords, self.nm_thresholds))
                self.reports.append({"file": p.f, **rep})
                line += " " + metrics.report_tokens(rep)
        self.n += 1
        self.emit(line)

    def write(self, p):
        """The output file, the error-map file and the normal-error-map file of an enqueued image, once its downloads have landed."""
        for d, t, write in ((self.out_dir, p.codes, self.fmt.write), (self.err_dir, p.emap, self.fmt.write),
                            (self.nm_dir, p.nmap, _write_angle_map)):
            if d and t is not None:
                p.event.synchronize()
                write(os.path.join(d, p.f), t.numpy())


def run_loop(model, dev, tdt, input_depth, input_color, label=None, out_dir=None, pipelined=True, emit=print, files=None,
             depth_bits=8, depth_max=65535, depth_unit=1.0, lr_depth=None, scale=None, self_ensemble=False, report=None, fill_holes=False,
             normalize=False, fill_guided=False, fill_sigma=FILL_SIGMA, baseline=None, jbu_sigma_s=JBU_SIGMA_S, jbu_sigma_r=FILL_SIGMA):
    """The test loop over every image pair.  Returns {"n", "rmse_mean", "ssim_mean", "seconds", "images_per_s"}.
    depth_bits=16: 16-bit depth and label files with codes 0 .. depth_max, outputs through metrics.postprocess_u16 into 16-bit
    PNGs, RMSE (metrics.masked_rmse_u16) in codes times depth_unit, SSIM of label / depth_max against out / depth_max.
    lr_depth (with scale; instead of input_depth): a directory of LOW-RESOLUTION depth maps, code 0 a hole -- the
    reader uploads the codes, and the main stream turns them into the depth input with codes_to_input ahead of the forward.
    self_ensemble: the forward of both loops becomes ensemble.self_ensemble(model, x, y) -- the mean over the eight
    D4 views, fp32 whatever the model's dtype -- and post-processing takes that fp32 map.
    report (needs label): {"thresholds": up to four codes, "edge_threshold": codes or None, "edge_radius": r,
    "error_maps": a directory or None} -- one more launch per image (metrics.depth_errors); every line gains the key=value
    tokens of metrics.depth_report (mad, rmse and max in codes times depth_unit), the error maps are written under the images'
    names, and the result gains "reports" (the per-image dicts, with "file") and "report_means" (metrics.report_means).
    report["normals"] (optional, and a report without it behaves to the byte as before): {"camera": the
    register.Camera of the label's grid, "radius", "tolerance", "tolerance_rel": metrics.normal_errors' (cloud's untuned defaults
    where left out), "thresholds": up to four angles in degrees, "error_maps": a directory or None} -- a second launch behind
    depth_errors (metrics.normal_errors), its words read back with the others; every line and every report dict gains the
    normal_* tokens of metrics.normal_report behind the depth tokens, and the angle maps are written as 8-bit PNGs of
    min(254, degrees), 255 where the pixel is not compared.  Right only where code is proportional to metric z.
    fill_holes, fill_guided, fill_sigma, normalize (need lr_depth): the preparation of the uploaded codes ahead of
    codes_to_input, prep.LrPrep's fields, run on the main stream in both loops.  fill_holes: the holes
    are filled by pull-push -- the network sees a dense input; fill_guided: by upsample.fill_holes_guided under
    fill_sigma, for which the loader also hands over the guidance as uint8 codes cropped to (h * scale, w * scale), one more
    upload of that many bytes.  normalize: the (filled) codes' own range [lo, hi] is stretched onto [1, top], the
    range stays on the device, and the post-processed output codes are mapped back (upsample.unstretch_codes) before anything
    else sees them: the metrics, the report, the error maps and the written files are in the files' own codes, and the label
    is never remapped.
    baseline (needs lr_depth, and model may be None): "bicubic" or "jbu" -- a classical upsampler in the network's
    place.  The prepared codes (fill -> stretch, unchanged) go through upsample.bicubic_upsample_codes, or through
    upsample.joint_bilateral_upsample under jbu_sigma_s (low-resolution pixels) and jbu_sigma_r (guidance codes), for which the
    loader hands over the guidance codes as for fill_guided; what comes out already is codes, so post-processing is skipped, and
    unstretching, metrics, report, error maps and files are the network path's.  tdt then only types the guidance nothing reads."""
    prep, jbu_sigma_s, jbu_sigma_r, files = _checked(model, input_depth, input_color, label, files, depth_bits, depth_max, lr_depth,
                                                     scale, self_ensemble, report, fill_holes, normalize, fill_guided, fill_sigma,
                                                     baseline, jbu_sigma_s, jbu_sigma_r)
    fmt = _format(depth_bits, depth_max, depth_unit)
    dm = fmt.depth_max
    # every load gives (x, y, label or None, h, w, guidance codes or None), guidance codes with fill_guided only; to_x(x or codes,
    # guidance codes) gives (the depth input, the range it was stretched by or None), and that range rides to the post-processing
    if lr_depth is not None:
        load = lambda f: _load_lr(lr_depth, input_color, label, f, tdt, scale, depth_bits, depth_max,            # noqa: E731
                                  with_guide=prep.fill_guided or baseline == "jbu")

        def to_x(c, g):                                 # [fill ->] [stretch ->] codes_to_input, or the baseline's codes
            c, lo_hi = prep.apply(c, g, scale, dm)
            if baseline is None:
                return codes_to_input(c, scale, tdt, dm), lo_hi
            up = (bicubic_upsample_codes(c, scale, dm) if baseline == "bicubic" else
                  joint_bilateral_upsample(c, g, scale, jbu_sigma_s, jbu_sigma_r, dm))
            return (up.view(torch.uint16) if depth_bits == 16 else up), lo_hi
    else:
        load = lambda f: (*_load_host(input_depth, input_color, label, f, tdt, depth_bits, depth_max), None)    # noqa: E731
        to_x = lambda x, g: (x, None)                                                                          # noqa: E731
    if baseline is not None:
        forward = lambda x, y: x                        # a baseline's output already is codes              # noqa: E731
    elif self_ensemble:
        from .ensemble import self_ensemble as _ensemble
        forward = lambda x, y: fmt.post_codes(_ensemble(model, x, y)[0, 0])                                    # noqa: E731
    else:
        forward = lambda x, y: fmt.post_codes(model(x, y)[0, 0])                                               # noqa: E731

    def codes_of(x, y, g):
        with torch.no_grad():
            x, lo_hi = to_x(x, g)
            o = forward(x, y)
        return o if lo_hi is None else unstretch_codes(o, lo_hi, dm)

    plan = _Plan(dev, fmt, load, codes_of, out_dir, emit, report)
    t0 = time.perf_counter()
    if pipelined:
        # READERS reader threads take every READERS-th image each (decoding two PNGs is the longest stage: 3.1 ms against a
        # 2.3 ms forward); uploads go on one side stream
        up_s = torch.cuda.Stream(device=dev)

        def step(loaded):
            p = plan.enqueue(loaded)
            return p, p

        run_pipeline(files, lambda f: plan.load(f, up_s), step, plan.settle, plan.write, READERS, "codon_infer")
    else:
        for f in files:
            p = plan.enqueue(plan.load(f))
            plan.write(p)
            plan.settle(p)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    n = plan.n
    res = {"n": n, "rmse_mean": plan.rm_sum / n if (label and n) else None, "ssim_mean": plan.ss_sum / n if (label and n) else None,
           "seconds": dt, "images_per_s": n / dt if dt > 0 else 0.0}
    if report is not None:
        res.update(reports=plan.reports, report_means=metrics.report_means(plan.reports))
    return res


def write_report_json(path, reports, means):
    """{"images": the per-image dicts, "means": {key: [mean, count]}} as STRICT JSON: a value over an empty set, nan in the
    dicts (an image without a discontinuity, or no --edge-threshold), is written as null."""
    import json
    clean = lambda v: None if isinstance(v, float) and math.isnan(v) else v                        # noqa: E731
    doc = {"images": [{k: clean(v) for k, v in r.items()} for r in reports],
           "means": {k: [clean(v[0]), v[1]] for k, v in means.items()}}
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, allow_nan=False)


def add_report_args(ap, prefix=""):
    """The parameter flags of the evaluation report, shared with codon_amd.train (prefix "val-")."""
    ap.add_argument(f"--{prefix}bad-thresholds", default=None, metavar="A,B,...",
                    help="report: up to four bad-pixel thresholds in codes; bad>T is the fraction of valid pixels off by more than T")
    ap.add_argument(f"--{prefix}edge-threshold", type=int, default=None, metavar="CODES",
                    help="report: split the error into an edge region and the rest; a valid label pixel with a valid 4-neighbour "
                         "more than this many codes away is a discontinuity (the sensor model's rule)")
    ap.add_argument(f"--{prefix}edge-radius", type=int, default=None, metavar="R",
                    help="report: the edge region is every valid pixel within R pixels (Chebyshev, 0..8, default 1) of a discontinuity")


def report_of(ap, a, prefix=""):
    """The run_loop report dict of the parsed parameter flags (without "error_maps"); refusals through ap.error."""
    key = prefix.replace("-", "_")
    thr, edge, rad = (getattr(a, key + n) for n in ("bad_thresholds", "edge_threshold", "edge_radius"))
    try:
        thr = tuple(int(t) for t in thr.split(",")) if thr else ()
    except ValueError:
        ap.error(f"--{prefix}bad-thresholds {thr!r}: integers in codes, separated by commas")
    if len(thr) > metrics.EVAL_MAX_THRESHOLDS or any(t < 0 for t in thr):
        ap.error(f"--{prefix}bad-thresholds takes at most {metrics.EVAL_MAX_THRESHOLDS} thresholds, none negative")
    if edge is not None and edge < 0:
        ap.error(f"--{prefix}edge-threshold {edge} must not be negative")
    if rad is not None and edge is None:
        ap.error(f"--{prefix}edge-radius needs --{prefix}edge-threshold")
    rad = 1 if rad is None else rad
    if not 0 <= rad <= metrics.EVAL_MAX_RADIUS:
        ap.error(f"--{prefix}edge-radius {rad} must lie in [0, {metrics.EVAL_MAX_RADIUS}]")
    return {"thresholds": thr, "edge_threshold": edge, "edge_radius": rad}


def add_normal_args(ap):
    """The flags of the normal report"""
    d = metrics.NORMAL_DEFAULTS
    ap.add_argument("--report-normals", action="store_true",
                    help="with --report and --calib: append the surface-normal angle error to the report -- normal_n, normal_coverage, "
                         "normal_mean, normal_rmse, normal_median in degrees and the fractions within --normal-thresholds -- between "
                         "the label's normals and the output's (cloud's integer normals, the output masked by the label's holes).  "
                         "Right only where code is proportional to metric z: not for disparity files")
    ap.add_argument("--calib", default=None, metavar="FILE",
                    help="report-normals: the rig's calibration, as python -m codon_amd.register reads it; the camera is the one the "
                         "LABEL's grid is on, without distortion, at least as large as the output")
    ap.add_argument("--camera", default=None, choices=("color", "depth"), help="report-normals: which camera of --calib (default color)")
    ap.add_argument("--normal-radius", type=int, default=None, metavar="R",
                    help=f"report-normals: a tangent spans the pixels R steps away, 1..8 (default {d['radius']}: cloud's, untuned)")
    ap.add_argument("--normal-tolerance", type=int, default=None, metavar="CODES",
                    help=f"report-normals: a far pixel counts when its code differs by at most R times this ... (default {d['tolerance']}: "
                         "cloud's, untuned)")
    ap.add_argument("--normal-tolerance-rel", type=float, default=None, metavar="F",
                    help=f"... plus this fraction of the smaller code (default {d['tolerance_rel']}: cloud's, untuned)")
    ap.add_argument("--normal-thresholds", default=None, metavar="A,B,...",
                    help="report-normals: up to four angles in degrees, multiples of 1/8; normal<T is the fraction of compared pixels "
                         "within T (default 11.25,22.5,30)")
    ap.add_argument("--normal-error-maps", default=None, metavar="DIR",
                    help="report-normals: write every image's angle map as an 8-bit PNG: min(254, degrees), 255 where the pixel is "
                         "not compared")


def normals_of(ap, a, top):
    """The parsed flags of the normal report as a dict (calib, camera, radius, tolerance, tolerance_rel, thresholds, error_maps),
    or None without --report-normals; refusals through ap.error.  top: the largest code"""
    from .codes import rel_q16
    names = ("calib", "camera", "normal_radius", "normal_tolerance", "normal_tolerance_rel", "normal_thresholds", "normal_error_maps")
    if not a.report_normals:
        for n in names:
            if getattr(a, n) is not None:
                ap.error(f"--{n.replace('_', '-')} needs --report-normals")
        return None
    if not a.report:
        ap.error("--report-normals needs --report")
    if a.calib is None:
        ap.error("--report-normals needs --calib")
    d = metrics.NORMAL_DEFAULTS
    radius = d["radius"] if a.normal_radius is None else a.normal_radius
    tol = d["tolerance"] if a.normal_tolerance is None else a.normal_tolerance
    rel = d["tolerance_rel"] if a.normal_tolerance_rel is None else a.normal_tolerance_rel
    if not 1 <= radius <= metrics.NORMAL_MAX_RADIUS:
        ap.error(f"--normal-radius {radius} must be in [1, {metrics.NORMAL_MAX_RADIUS}]")
    if not 0 <= tol <= top:
        ap.error(f"--normal-tolerance {tol} must be in [0, {top}], the largest code")
    try:
        rel_q16("infer", rel)
    except ValueError:
        ap.error(f"--normal-tolerance-rel {rel} must be in [0, 1)")
    thr = metrics.NORMAL_THRESHOLDS
    if a.normal_thresholds is not None:
        try:
            thr = tuple(float(t) for t in a.normal_thresholds.split(","))
        except ValueError:
            ap.error(f"--normal-thresholds {a.normal_thresholds!r}: degrees, separated by commas")
        try:
            thr = metrics.normal_thresholds(thr, "infer")
        except ValueError as e:
            ap.error(f"--normal-thresholds {a.normal_thresholds!r}: {e}")
    if a.normal_error_maps is not None:
        inputs = {os.path.abspath(d_) for d_ in (a.input_depth, a.lr_depth, a.input_color, a.label) if d_}
        if os.path.abspath(a.normal_error_maps) in inputs:
            ap.error("--normal-error-maps is a directory of inputs: the maps would overwrite them")
    return {"calib": a.calib, "camera": a.camera or "color", "radius": radius, "tolerance": tol, "tolerance_rel": rel,
            "thresholds": thr, "error_maps": a.normal_error_maps}


def parse_args(argv=None):
    """-> (the parsed flags, the parser), every refusal that needs neither a file nor the GPU made through ap.error; the flags gain
    report_opts (run_loop's report dict, or None), prep (prep.LrPrep) and normals (normals_of's dict, or None)"""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=4, choices=[4, 8, 16])
    ap.add_argument("--input-depth", default=None, help="depth maps already at the output size (this or --lr-depth)")
    ap.add_argument("--lr-depth", default=None,
                    help="LOW-RESOLUTION depth maps as a sensor writes them, code 0 a hole: upsampled by --scale on the device "
                         "with the training degradation's own hole-aware bicubic; guidance and label are cropped to "
                         "(h * scale, w * scale)")
    add_prep_args(ap, {
        "fill_holes": "with --lr-depth: fill the holes of every low-resolution map on the device by pull-push (the mean of "
                      "the valid pixels up a pyramid, a 9/3/3/1 mix back down; integers, bit-exact) before it is upsampled, "
                      "so that the network sees a dense input; valid pixels are untouched",
        "fill_guided": "with --fill-holes: guidance-aware filling -- a hole weighs the pixels it is filled from by how close "
                       "their guidance (the --input-color image, box-averaged over the pixel) is to its own, so a hole beside "
                       "an occlusion edge takes its own side's depth instead of a ramp across the edge (integers, bit-exact; "
                       "DESIGN 12.11)",
        "normalize": "with --lr-depth: per-image range normalisation -- the valid codes [lo, hi] of every low-resolution "
                     "map (after --fill-holes) are stretched onto [1, top] of the code grid on the device, holes stay "
                     "holes, and the output codes are mapped back before they are measured and written (integers, "
                     "bit-exact; DESIGN 12.10)"})
    ap.add_argument("--input-color", required=True)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--weights", default=None, help="X4.pth-style checkpoint; random reference init if absent")
    ap.add_argument("--dtype", default="f16", choices=["f32", "bf16", "f16"],
                    help="the reference script runs .half(); fp16 and bf16 carry 11 and 8 significant bits, so f32 is the "
                         "sensible choice for 16-bit data (--depth-bits 16)")
    ap.add_argument("--ema", action="store_true", help="load the EMA weights of a codon_amd.train --ema checkpoint")
    ap.add_argument("--self-ensemble", action="store_true",
                    help="geometric self-ensemble: run the network on the eight flips and rotations of every pair (two forwards of "
                         "four views each), undo each on the output and average -- eight forwards' worth of convolution per "
                         "image.  The mean is fp32 whatever --dtype is, so an f16 or bf16 run now post-processes an fp32 map "
                         "(clip, scale and truncate in fp32) where it otherwise post-processes the 16-bit output itself")
    ap.add_argument("--baseline", default=None, choices=list(BASELINES),
                    help="with --lr-depth: run a classical upsampler in the network's place (DESIGN 12.14) -- bicubic: the "
                         "hole-aware bicubic that builds the network's input, as codes; jbu: joint bilateral upsampling (Kopf et "
                         "al. 2007) under the --input-color image.  No model is built and --dtype is not looked at; "
                         "--fill-holes, --fill-guided and --normalize prepare the map as they do for the network, and the "
                         "metrics, the report and the files are the network path's (integers, bit-exact)")
    ap.add_argument("--jbu-sigma-s", type=float, default=None, metavar="F",
                    help=f"with --baseline jbu: the spatial sigma in low-resolution pixels (default {JBU_SIGMA_S}, untuned)")
    ap.add_argument("--jbu-sigma-r", type=float, default=None, metavar="CODES",
                    help=f"with --baseline jbu: the range sigma in guidance codes (default {FILL_SIGMA}, untuned)")
    ap.add_argument("--serial", action="store_true", help="the reference's own serial loop (decode, upload, forward, download, "
                                                          "encode one after the other per image) instead of the pipeline")
    ap.add_argument("--depth-bits", type=int, default=8, choices=[8, 16],
                    help="16: depth maps and labels are 16-bit PNGs of codes 0 .. --depth-max (0 a hole), and so are the outputs")
    ap.add_argument("--depth-max", type=int, default=None, help="with --depth-bits 16: the code of 1.0 (default 65535)")
    ap.add_argument("--depth-unit", type=float, default=1.0,
                    help="with --depth-bits 16: the printed RMSE is in codes times this (0.1: centimetres from millimetre codes)")
    ap.add_argument("--report", action="store_true",
                    help="with --label: append the evaluation suite's key=value tokens (MAD, RMSE, max, bad-pixel rates, delta "
                         "accuracies, edge / flat split) to every image's line and print a last line of their means")
    add_report_args(ap)
    ap.add_argument("--report-json", default=None, metavar="FILE", help="report: write the per-image values and the means here (JSON; a value over an empty set is null)")
    ap.add_argument("--error-maps", default=None, metavar="DIR",
                    help="report: write every image's error map |label - output| (0 at holes) as a PNG of the data's depth")
    add_normal_args(ap)
    a = ap.parse_args(argv)
    if a.report and not a.label:
        ap.error("--report needs --label")
    if not a.report:
        for n in ("bad_thresholds", "edge_threshold", "edge_radius", "report_json", "error_maps"):
            if getattr(a, n) is not None:
                ap.error(f"--{n.replace('_', '-')} needs --report")
    report = {**report_of(ap, a), "error_maps": a.error_maps} if a.report else None
    if (a.input_depth is None) == (a.lr_depth is None):
        ap.error("exactly one of --input-depth and --lr-depth is required")
    if a.fill_holes and a.lr_depth is None:
        ap.error("--fill-holes needs --lr-depth")
    prep = prep_of(ap, a, a.fill_holes, "--fill-holes (and with it --lr-depth)")
    if a.normalize and a.lr_depth is None:
        ap.error("--normalize needs --lr-depth (it is refused with --input-depth: only low-resolution code planes are normalised)")
    if a.baseline is not None:
        if a.input_depth is not None or a.lr_depth is None:
            ap.error("--baseline needs --lr-depth (it is refused with --input-depth: a baseline upsamples low-resolution code planes)")
        for flag, given in (("--weights", a.weights is not None), ("--ema", a.ema), ("--self-ensemble", a.self_ensemble)):
            if given:
                ap.error(f"--baseline is refused with {flag} (no network runs)")
    if a.ema and not a.weights:
        ap.error("--ema needs --weights")
    for flag, v in (("--jbu-sigma-s", a.jbu_sigma_s), ("--jbu-sigma-r", a.jbu_sigma_r)):
        if v is not None and a.baseline != "jbu":
            ap.error(f"{flag} needs --baseline jbu")
        if v is not None and not (0.0 < v < float("inf")):
            ap.error(f"{flag} {v} must be positive")
    if a.depth_bits != 16 and (a.depth_max is not None or a.depth_unit != 1.0):
        ap.error("--depth-max and --depth-unit belong to --depth-bits 16")
    a.depth_max = 65535 if a.depth_max is None else a.depth_max
    if not 1 <= a.depth_max <= 65535:
        ap.error(f"--depth-max {a.depth_max} must lie in [1, 65535]")
    a.report_opts, a.prep = report, prep
    a.normals = normals_of(ap, a, a.depth_max if a.depth_bits == 16 else 255)
    return a, ap


def main(argv=None):
    a, ap = parse_args(argv)
    report, prep = a.report_opts, a.prep
    if a.normals is not None:                           # the camera of the label's grid, read before the GPU is asked for
        from .register import Calibration
        try:
            cal = Calibration.from_json(a.normals["calib"])
        except (OSError, ValueError) as e:
            ap.error(f"--calib {a.normals['calib']}: {e}")
        cam = cal.color if a.normals["camera"] == "color" else cal.depth
        if any(cam.dist):
            ap.error(f"--calib {a.normals['calib']}: {a.normals['camera']}.dist {cam.dist!r} is not zero: undistort the images first "
                     "(python -m codon_amd.undistort --calib-out ...)")
        report = {**report, "normals": {**{k: v for k, v in a.normals.items() if k != "calib"}, "camera": cam}}
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found, codon_amd has no CPU path")          # test.py:37-38
    dev = torch.device("cuda:0")
    if a.baseline is not None:                          # no network: nothing is constructed, --dtype is not looked at
        model, tdt = None, torch.float32
        extra = {"baseline": a.baseline,
                 **({"jbu_sigma_s": JBU_SIGMA_S if a.jbu_sigma_s is None else a.jbu_sigma_s,
                     "jbu_sigma_r": FILL_SIGMA if a.jbu_sigma_r is None else a.jbu_sigma_r} if a.baseline == "jbu" else {})}
    else:
        model = (CODONNet16 if a.scale == 16 else CODONNet)()
        if a.weights:
            print("loaded epoch", io.load_checkpoint(a.weights, model, ema=a.ema))
        else:
            print("WARNING: no --weights given (the reference's X*.pth are not shipped): random init")
        tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
        model = model.to(dev).to(tdt).eval()
        extra = {}
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    for d in (a.error_maps, a.normals and a.normals["error_maps"]):
        if d:
            os.makedirs(d, exist_ok=True)
    r = run_loop(model, dev, tdt, a.input_depth, a.input_color, a.label, a.out, pipelined=not a.serial,
                 depth_bits=a.depth_bits, depth_max=a.depth_max, depth_unit=a.depth_unit,
                 **({"self_ensemble": True} if a.self_ensemble else {}), **({"report": report} if report else {}),
                 **({"lr_depth": a.lr_depth, "scale": a.scale} if a.lr_depth else {}), **prep.set_options(), **extra)
    print(r["n"])
    if a.label and r["n"]:
        print(r["rmse_mean"], r["ssim_mean"])
    if report and r["n"]:
        print("mean " + metrics.report_tokens(r["report_means"]))
    if a.report_json:
        write_report_json(a.report_json, r.get("reports", []), r.get("report_means", {}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
