"""python -m codon_amd.train -- fine-tune CODONNet on a directory of depth maps and grey guidance images.

The reference ships only a test script and weights; its depth inputs were degraded offline (bicubic down, bicubic up, saved
as 8-bit PNGs: the reference's CODON_X4/test.py:70-79,116-123) by a script it does not ship.  Here every training batch is
built ON THE DEVICE from HR depth maps and guidance images uploaded once (codon_amd/csrc/train_data.hip):
    random crop + D4 op (crop, u8 -> fp32)  ->  antialiased bicubic x1/s  ->  bicubic xs (upsample.hip)  ->  8-bit quantise
The degradation is a definition of this project, NOT pinned to the reference (its script is not shipped); it is restated in
numpy in tests/train_data_ref.py and the two agree bit for bit.  --depth-bits 16: depth maps and labels are
16-bit PNGs of codes 0 .. --depth-max (0 a hole, value = code / depth-max, guidance stays 8-bit); the crop reads u16 planes
through a 65 536-entry table and the last step quantises onto the data set's own code grid (tests/train_data16_ref.py).
--fill-holes: the holes of the low-resolution maps -- real ones, or the synthetic ones of --degrade-holes -- are
filled on the device by pull-push before they are upsampled, exactly as `codon_amd.infer --lr-depth --fill-holes` fills them.
--normalize: per-image range normalisation -- once the pool is on the device every record's codes are stretched in
place from their own valid range onto the whole code grid, exactly as `codon_amd.infer --lr-depth --normalize` stretches them.
--train-lr-depth DIR: REAL pairs -- a sensor's low-resolution map per pair, paired by file name; nothing is
degraded, one launch (codon_train_crops_lr) builds x, y and t, and x is the crop of what `codon_amd.infer --lr-depth` builds from
the whole low-resolution file, bit for bit (tests/train_lr_ref.py).
--sensor-noise / --sensor-noise-quad / --sensor-dropout / --sensor-edge-dropout: a sensor model on the synthetic
low-resolution map -- range noise from a Gaussian table and per-pixel dropout, both driven by Philox4x32-10 of (pixel, sample
of the global batch, step; --seed), so that any number of ranks and a resumed run see the same maps (tests/sensor_ref.py).

One step: GradSync.zero_grad -> synthesize -> forward -> L1SSIMLoss(out.float(), t) (--mask-holes: MaskedL1SSIMLoss, which
leaves the target's holes -- code 0 -- out of the loss; --train-label: targets from a third directory) -> GradSync.backward ->
all_reduce_grads -> FlatAdam.step, the sequence of bench.py's training leg (optionally with gradient clipping, skipping of
non-finite steps, EMA weights and a learning-rate schedule, all on the device: DESIGN 12.1).  Under torchrun every rank
draws the whole global batch from the same seeded generator and keeps its shard (codon_amd.dist.shard_batch); the loss is
read back on log steps only.  Checkpoints are {"epoch": step, "model", "optimizer", "rng", "args"}: io.load_checkpoint and
`python -m codon_amd.infer --weights` read them as they are (with --ema also "model_ema", read by `infer --ema`), and --resume
continues a run bit for bit.
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import math
import os
import time

import numpy as np
import torch

from . import CODONNet, CODONNet16, io
from . import _lib as L
from . import ops
from .infer import add_report_args, report_of, run_loop
from .io import check_depth_max, list_pairs, read_depth_plane
from .metrics import report_tokens
from .codes import code_table, on_device
from .upsample import (_fill_launch, down_weights, gauss_table, lut16, phase_weights, u8_lut)      # noqa: F401 (lut16: for importers)
from .prep import LrPrep, add_prep_args, prep_of
from .upsample import FILL_SIGMA, code_range, stretch_codes
# the options that change a run's trajectory: the table of checkpoint keys, its views, the record and the command line's mappings
from .options import (DEGRADE_DEFAULTS, DEPTH_DEFAULTS, FILL_DEFAULTS, GUIDED_DEFAULTS, LR_DEFAULTS, NORM_DEFAULTS,      # noqa: F401
                      RESUME_ALL_DEFAULTS, RESUME_ALL_KEYS, RESUME_DEFAULTS, RESUME_KEYS, RESUME_TABLE, SENSOR_DEFAULTS,
                      RunOptions, SensorModel, fit_kwargs, run_args, sensor_of)

DTYPES = {"bf16": torch.bfloat16, "f32": None}
MAX_REDRAWS = 64                                    # draw(min_valid=): per sample, before it gives up
LR_SCHEDULES = ("constant", "cosine")


# ---- the dataset --------------------------------------------------------------------------------------------------------------

def record_layout(bits: int, label: bool, lr_scale: int, h: int, w: int) -> dict:
    """Where the planes of one pool record sit, as byte offsets from its start, and the bytes they take ("size"): the mirror
    of record_layout in csrc/train_record.h (the six layouts are tabled in DESIGN 12.3).  The depth plane (h*w codes of
    `bits` bits) comes first; the label plane (h*w codes) or the low-resolution plane ((h/lr_scale)*(w/lr_scale) codes; 0: none)
    -- never both -- starts at byte 2*h*w; the guidance is h*w u8, second in an 8-bit record and last in a 16-bit one.  u16
    planes are little-endian and start at even bytes: the pool pads a 16-bit record of odd size by a byte "size" leaves out."""
    hw = h * w
    extra = (hw if label else 0) + ((h // lr_scale) * (w // lr_scale) if lr_scale else 0)
    if bits == 16:
        return {"depth": 0, "guide": 2 * hw + 2 * extra, "label": 2 * hw, "lr": 2 * hw, "size": 3 * hw + 2 * extra}
    return {"depth": 0, "guide": hw, "label": 2 * hw, "lr": 2 * hw, "size": 2 * hw + extra}


class TrainSet:
    """Every (depth, guidance) pair of two directories, paired by file name (io.list_pairs), read with io.read_depth_plane and
    io.read_gray and cropped to their common size (as infer._load_host does), in ONE flat uint8 pool on `device`: pair i's
    record at offsets[i], its planes where record_layout says.  Uploaded once; a step reads nothing from the host.  `crop`:
    refuse images smaller than it.  `label_dir`: a third plane per pair, the label (the target, which may carry holes coded 0
    that the depth map -- the degradation's source -- has filled in); every pair needs a namesake there.
    depth_bits=16: depth maps and labels are 16-bit PNGs of codes 0 .. depth_max (0 a hole, v = c / depth_max);
    the pool stays a BYTE pool of records at even offsets.  With depth_bits=8 a 16-bit depth or label file is refused (it used
    to be clipped at 255), with 16 an 8-bit one.
    `lr_dir` with `scale`: real pairs -- every pair has a namesake there, a LOW-RESOLUTION map of codes as a
    sensor writes it (0 a hole), read through read_depth_plane under the set's bit depth.  Its (h, w) fixes the HR size
    (h * scale, w * scale), to which depth map and guidance are cropped top-left (a smaller one is refused by name: the rule
    of `infer --lr-depth`); `sizes` holds the HR sizes.  The depth map is the target and nothing is degraded, so lr_dir
    excludes label_dir.  has_lr, lr_scale say so (False, None otherwise).
    `fill_holes`, `fill_guided`, `fill_sigma`, `normalize`: the preparation (prep.LrPrep's fields; kept as `prep`
    and readable under their names), done ONCE, when the pool is on the device, so that a step costs nothing extra.
    fill_holes (needs lr_dir): the low-resolution plane of every record is filled by pull-push from the WHOLE file, so
    that x stays the crop of what `infer --lr-depth --fill-holes` builds from that file; the target plane is untouched.
    fill_guided: by upsample.fill_holes_guided under fill_sigma, with the record's own guide plane read in place.
    normalize (excludes label_dir): after the filling, every record's code planes are stretched IN PLACE.  With
    lr_dir the range is that of the (filled) low-resolution plane of the WHOLE file, as `infer --lr-depth --normalize` takes it;
    it stretches that plane and, clamped, the HR target plane.  Without lr_dir the depth plane is stretched by its own range."""

    def __init__(self, depth_dir: str, color_dir: str, device, crop: int = None, label_dir: str = None, depth_bits: int = 8,
                 depth_max: int = 65535, lr_dir: str = None, scale: int = None, fill_holes: bool = False,
                 normalize: bool = False, fill_guided: bool = False, fill_sigma: float = FILL_SIGMA):
        if depth_bits not in (8, 16):
            raise ValueError(f"TrainSet: depth_bits {depth_bits!r} (8 or 16)")
        check_depth_max(depth_max)
        self.depth_bits, self.depth_max = depth_bits, int(depth_max)
        self.has_lr, self.lr_scale = lr_dir is not None, None
        if normalize and label_dir is not None:
            raise ValueError("TrainSet: normalize and label_dir exclude each other (a label plane has no range of its own "
                             "to be stretched by)")
        self.prep = LrPrep.checked("TrainSet", fill_holes, fill_guided, fill_sigma, normalize, lr=("lr_dir", self.has_lr),
                                   top=self.depth_max if depth_bits == 16 else 255, normalize_needs_lr=False)
        if self.has_lr:
            if scale not in (4, 8, 16):
                raise ValueError(f"TrainSet: lr_dir needs scale 4, 8 or 16 (got {scale!r})")
            if label_dir is not None:
                raise ValueError("TrainSet: lr_dir and label_dir exclude each other (with low-resolution maps the depth "
                                 "directory is the target)")
            self.lr_scale = int(scale)
        self.files = list_pairs(depth_dir, color_dir)
        if not self.files:
            raise ValueError(f"TrainSet: no file of {color_dir} has a namesake in {depth_dir}")
        self.has_label = label_dir is not None
        self.planes = 3 if self.has_label else 2
        deep = depth_bits == 16
        chunks, offsets, sizes, off = [], [], [], 0
        for f in self.files:
            planes = {}
            for name, d in (("lr", lr_dir), ("depth", depth_dir), ("label", label_dir)):
                if d is None:
                    continue
                if name != "depth" and not os.path.isfile(os.path.join(d, f)):
                    raise ValueError(f"TrainSet: {f} has no namesake in {d}")
                planes[name] = read_depth_plane(os.path.join(d, f), depth_bits, self.depth_max)
            planes["guide"] = io.read_gray(os.path.join(color_dir, f))
            lr = planes.pop("lr", None)
            if lr is None:
                h, w = min(p.shape[0] for p in planes.values()), min(p.shape[1] for p in planes.values())
            else:                                       # the low-resolution map fixes the size
                h, w = lr.shape[0] * self.lr_scale, lr.shape[1] * self.lr_scale
                for d, p in ((depth_dir, planes["depth"]), (color_dir, planes["guide"])):
                    if p.shape[0] < h or p.shape[1] < w:
                        raise ValueError(f"{os.path.join(d, f)}: {p.shape[0]}x{p.shape[1]}, smaller than the {h}x{w} that "
                                         f"{os.path.join(lr_dir, f)} gives at x{self.lr_scale}")
            if crop is not None and (h < crop or w < crop):
                raise ValueError(f"TrainSet: {f} is {h}x{w}, smaller than the {crop}x{crop} crop")
            planes = {name: p[:h, :w] for name, p in planes.items()}
            if lr is not None:
                planes["lr"] = lr
            lay = record_layout(depth_bits, self.has_label, self.lr_scale or 0, h, w)
            rec = np.zeros(lay["size"] + (lay["size"] % 2 if deep else 0), dtype=np.uint8)      # the next u16 record starts even
            for name, p in planes.items():
                raw = np.ascontiguousarray(p).astype("<u2" if deep and name != "guide" else np.uint8).reshape(-1).view(np.uint8)
                rec[lay[name]:lay[name] + raw.size] = raw
            chunks.append(rec)
            offsets.append(off)
            sizes.append((h, w))
            off += rec.size
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.sizes = np.asarray(sizes, dtype=np.int64)
        self.pool = torch.from_numpy(np.concatenate(chunks)).to(device)
        self._integrals = None
        dm = self.depth_max if deep else None
        records = list(zip(self.offsets.tolist(), self.sizes.tolist()))
        if self.prep.fill_holes:                        # every record filled, then every record stretched
            for off, (h, w) in records:
                lr = self.plane(off, "lr", h, w)
                lr.copy_(self.prep.fill(lr, self.plane(off, "guide", h, w), self.lr_scale, dm))
        if self.prep.normalize:
            for off, (h, w) in records:
                planes = [self.plane(off, name, h, w) for name in (("depth", "lr") if self.has_lr else ("depth",))]
                lo_hi = code_range(planes[-1])
                for p in planes:                        # the target plane of real pairs is clamped into the map's range
                    stretch_codes(p, dm, lo_hi, out=p)

    fill_holes, fill_guided, fill_sigma, normalize = (property(lambda self, n=n: getattr(self.prep, n)) for n in
                                                      ("fill_holes", "fill_guided", "fill_sigma", "normalize"))

    def plane_offset(self, off: int, name: str, h: int, w: int) -> int:
        """Where plane `name` ("depth", "guide", "label", "lr") of the (h, w) record at pool offset `off` starts, in bytes"""
        return off + record_layout(self.depth_bits, self.has_label, self.lr_scale or 0, h, w)[name]

    def plane(self, off: int, name: str, h: int, w: int) -> torch.Tensor:
        """The device view of that plane in the pool: (h, w) -- the low-resolution plane (h / lr_scale, w / lr_scale) -- uint8, or
        the u16 bits of a code plane of a 16-bit set as int16"""
        ph, pw = (h // self.lr_scale, w // self.lr_scale) if name == "lr" else (h, w)
        lo = self.plane_offset(off, name, h, w)
        if self.depth_bits == 8 or name == "guide":
            return self.pool[lo:lo + ph * pw].view(ph, pw)
        return self.pool[lo:lo + 2 * ph * pw].view(torch.int16).view(ph, pw)

    def __len__(self):
        return len(self.files)

    def valid_integrals(self) -> dict:
        """{pool offset: (H+1, W+1) int32 integral image of validity (code != 0)} of the TARGET plane -- the label if there is
        one, else the depth map.  Built on first use (masking in force) from one read of the pool, kept on the host: a crop's
        valid count is then four lookups and no step reads the device for it."""
        if self._integrals is None:
            pool = self.pool.cpu().numpy()
            wide = self.depth_bits // 8
            self._integrals = {}
            for off, (h, w) in zip(self.offsets.tolist(), self.sizes.tolist()):
                lo = self.plane_offset(off, "label" if self.has_label else "depth", h, w)
                v = pool[lo:lo + wide * h * w].view("<u2" if wide == 2 else np.uint8).reshape(h, w) != 0
                ii = np.zeros((h + 1, w + 1), dtype=np.int32)
                ii[1:, 1:] = v.cumsum(0, dtype=np.int32).cumsum(1, dtype=np.int32)
                self._integrals[off] = ii
        return self._integrals


def valid_counts(trainset: TrainSet, descs: np.ndarray, crop: int) -> np.ndarray:
    """Valid pixels of each descriptor's crop (a D4 op moves none in or out), from the host-side integral images."""
    ii = trainset.valid_integrals()
    out = np.empty(len(descs), dtype=np.int64)
    for b, (off, _, _, y0, x0, _) in enumerate(np.asarray(descs, dtype=np.int64).tolist()):
        t = ii[off]
        out[b] = int(t[y0 + crop, x0 + crop]) - int(t[y0, x0 + crop]) - int(t[y0 + crop, x0]) + int(t[y0, x0])
    return out


def check_min_valid(who: str, min_valid: float, mask_holes: bool):
    """draw's threshold is a fraction, and means something under the masked loss only (draw: always; fit: with mask_holes)"""
    if not 0.0 <= min_valid <= 1.0 or (min_valid > 0 and not mask_holes):
        raise ValueError(f"{who}: min_valid {min_valid} must lie in [0, 1]" + ("" if mask_holes else " and needs mask_holes"))


def draw(rng: np.random.Generator, trainset: TrainSet, batch: int, crop: int, rank: int = 0, world: int = 1,
         min_valid: float = 0.0) -> np.ndarray:
    """This rank's share of one global batch: (batch/world, 6) int64 rows (pool offset, H, W, y0, x0, D4 op).  Every rank
    draws the WHOLE batch (the generators stay in step) and keeps shard_batch(batch, rank, world).
    min_valid > 0: a sample whose crop holds fewer than min_valid * crop^2 valid pixels (TrainSet.valid_integrals) is drawn
    again from the same generator -- index, y0, x0 and op together, at most MAX_REDRAWS times, then ValueError.  With
    min_valid == 0 the generator is consumed exactly as without the option."""
    from .dist import shard_batch
    if batch < 1 or world < 1 or batch % world:
        raise ValueError(f"draw: a batch of {batch} does not split evenly over {world} ranks")
    if crop < 1 or (trainset.sizes < crop).any():
        raise ValueError(f"draw: crop {crop} does not fit the smallest image "
                         f"({int(trainset.sizes[:, 0].min())}x{int(trainset.sizes[:, 1].min())})")
    check_min_valid("draw", min_valid, True)
    idx = rng.integers(0, len(trainset.offsets), size=batch)
    hw = trainset.sizes[idx]
    y0 = rng.integers(0, hw[:, 0] - crop + 1)
    x0 = rng.integers(0, hw[:, 1] - crop + 1)
    op = rng.integers(0, 8, size=batch)
    d = np.stack([trainset.offsets[idx], hw[:, 0], hw[:, 1], y0, x0, op], axis=1).astype(np.int64)
    if min_valid > 0:
        need = min_valid * crop * crop
        for b in np.flatnonzero(valid_counts(trainset, d, crop) < need).tolist():
            for _ in range(MAX_REDRAWS):
                i = int(rng.integers(0, len(trainset.offsets)))
                h, w = trainset.sizes[i].tolist()
                d[b] = [trainset.offsets[i], h, w, rng.integers(0, h - crop + 1), rng.integers(0, w - crop + 1),
                        rng.integers(0, 8)]
                if valid_counts(trainset, d[b:b + 1], crop)[0] >= need:
                    break
            else:
                raise ValueError(f"draw: no crop with at least min_valid = {min_valid} of its {crop}x{crop} pixels valid in "
                                 f"{MAX_REDRAWS} redraws of sample {b}: lower the threshold")
    lo, hi = shard_batch(batch, rank, world)
    return d[lo:hi]


def check_sensor(who: str, trainset: TrainSet, sensor: SensorModel, degrade_holes: bool):
    if trainset.has_lr:
        raise ValueError(f"{who}: a sensor model does not go with a TrainSet of low-resolution maps (nothing is degraded: the "
                         "maps carry their sensor's own noise and holes)")
    if sensor.drops and not degrade_holes:
        raise ValueError(f"{who}: sensor dropout needs degrade_holes (without the masked upsample a dropped pixel would ring "
                         "instead of being left out)")


def check_fill(who: str, trainset: TrainSet, fill_holes: bool, degrade_holes: bool):
    if fill_holes and not (degrade_holes or (trainset.has_lr and trainset.fill_holes)):
        raise ValueError(f"{who}: fill_holes needs degrade_holes, or a TrainSet of low-resolution maps built with fill_holes "
                         "(the unmasked degradation has no holes to fill)")


def synthesize(trainset: TrainSet, descs: np.ndarray, scale: int, crop: int, degrade_holes: bool = False,
               return_lr: bool = False, sensor: SensorModel = None, step: int = 0, first_sample: int = 0,
               fill_holes: bool = False):
    """(x, y, t), each (B,1,crop,crop) fp32 on the pool's device: the network's depth input (crop -> bicubic down by `scale`
    -> bicubic up -> 8-bit), the guidance and the HR target.  Four launches on the caller's stream, no host synchronisation.
    A TrainSet with labels: x is degraded from the depth plane, t comes from the label plane (codon_train_crops_labeled).
    A 16-bit TrainSet: codon_train_crops_u16 (labeled or not) and codon_quantize_levels onto the set's own code grid, the
    down and up kernels between them unchanged -- four launches as well.
    degrade_holes: the source's holes (0.0) are left out of both bicubics instead of being smeared through them --
    codon_bicubic_downsample_masked (whose result is a low-resolution map on the code grid, holes 0.0, as a sensor's file holds
    it) and codon_bicubic_upsample_masked take the place of the down and up launches, the quantise launch follows unchanged:
    four launches still, no host synchronisation; x is bit for bit what infer.codes_to_input builds from that map's codes.
    return_lr: (x, y, t, lr) with lr the (B,1,crop/scale,crop/scale) low-resolution map.
    A TrainSet with low-resolution maps (lr_dir): ONE launch, codon_train_crops_lr, and none of the others -- t and
    y are the crop of the depth map and the guidance, x is the window, under the D4 op, of what infer.codes_to_input builds from
    the WHOLE low-resolution file in fp32.  `scale` must be the set's lr_scale; degrade_holes and return_lr are refused (there
    is no degradation to mask and no per-crop low-resolution map to return).
    sensor: ONE more launch, codon_lr_sensor, between the down and the up launch of either path -- five launches,
    still no host synchronisation.  Pixel (y, x) of sample b draws its noise and dropout from Philox4x32-10 of the counter
    (y * p + x, first_sample + b, step, 0) under the model's seed: `step` is the training step and `first_sample` the index of
    descs[0] in the GLOBAL batch (this rank's shard start).  The up launch reads the new map and return_lr returns it; on the
    masked path the map stays on the code grid and x stays what infer.codes_to_input builds from its codes.  Dropout needs
    degrade_holes, and a TrainSet with low-resolution maps refuses a model.
    fill_holes: with degrade_holes ONE more launch, codon_fill_holes in its fp32-on-the-grid format, between the
    sensor launch (or the down launch) and the masked up launch: the low-resolution map's holes are filled by pull-push, the up
    and the quantise launch stay as they are, return_lr returns the filled map, and x is what infer.codes_to_input builds from
    upsample.fill_holes of that map's codes.  With a TrainSet of low-resolution maps built with fill_holes it changes nothing
    (the pool is already filled).  Anything else is refused: the unmasked degradation has no holes."""
    check_fill("synthesize", trainset, fill_holes, degrade_holes)
    if sensor is not None:
        check_sensor("synthesize", trainset, sensor, degrade_holes)
        if not 0 <= step < 1 << 32 or not 0 <= first_sample <= (1 << 32) - len(descs):
            raise ValueError(f"synthesize: step {step} and first_sample {first_sample} must fit 32 bits")
        if crop // scale > 512:
            raise ValueError(f"synthesize: the sensor model takes low-resolution maps up to 512 (crop {crop} at x{scale})")
    lib = L.load()
    B = len(descs)
    if not 1 <= B <= L.TRAIN_MAX_BATCH:
        raise ValueError(f"synthesize: {B} samples per launch (1..{L.TRAIN_MAX_BATCH})")
    if crop % scale or crop // scale < 4:
        raise ValueError(f"synthesize: crop {crop} must be a multiple of the scale {scale} and at least 4 * scale")
    if degrade_holes and crop > 1024:
        raise ValueError(f"synthesize: degrade_holes takes crops up to 1024 (crop {crop})")
    if trainset.has_lr:
        if scale != trainset.lr_scale:
            raise ValueError(f"synthesize: scale {scale} with a TrainSet of x{trainset.lr_scale} low-resolution maps")
        if degrade_holes or return_lr:
            raise ValueError("synthesize: degrade_holes and return_lr do not go with a TrainSet of low-resolution maps "
                             "(nothing is degraded, and there is no per-crop low-resolution map)")
    dev = trainset.pool.device
    d = L.CropDesc()
    d.n, d.crop = B, crop
    for b, (off, h, w, y0, x0, op) in enumerate(np.asarray(descs, dtype=np.int64).tolist()):
        s = d.s[b]
        s.offset, s.height, s.width, s.y0, s.x0, s.op = off, h, w, y0, x0, op
    deep = trainset.depth_bits == 16
    tab, top = code_table(trainset.depth_bits, trainset.depth_max, dev)      # the depth codes' table (the set's own grid)
    lut = on_device("lut", u8_lut, dev)                                     # the guidance's
    wup = on_device(("up", scale), lambda: phase_weights(scale), dev)
    P_ = C.c_void_p
    pool = (C.byref(d), P_(trainset.pool.data_ptr()), trainset.pool.numel())
    t = torch.empty((B, 1, crop, crop), dtype=torch.float32, device=dev)
    y, x = torch.empty_like(t), torch.empty_like(t)
    with ops._on(dev):
        st = ops._stream(dev)
        if trainset.has_lr:
            L.check(lib.codon_train_crops_lr(*pool, scale, trainset.depth_bits, P_(tab.data_ptr()), top, P_(lut.data_ptr()),
                                             P_(wup.data_ptr()), P_(x.data_ptr()), P_(y.data_ptr()), P_(t.data_ptr()), st),
                    "train_crops_lr")
            return x, y, t
        wdown = on_device(("down", crop, scale), lambda: down_weights(crop, scale), dev)
        p = crop // scale
        src = torch.empty_like(t) if trainset.has_label else t        # what the degradation reads
        lr = torch.empty((B, 1, p, p), dtype=torch.float32, device=dev)
        if deep:
            L.check(lib.codon_train_crops_u16(*pool, P_(tab.data_ptr()), P_(lut.data_ptr()), P_(src.data_ptr()),
                                              P_(y.data_ptr()), P_(t.data_ptr()) if trainset.has_label else None, st),
                    "train_crops_u16")
        elif trainset.has_label:
            L.check(lib.codon_train_crops_labeled(*pool, P_(lut.data_ptr()), P_(src.data_ptr()), P_(y.data_ptr()),
                                                  P_(t.data_ptr()), st), "train_crops_labeled")
        else:
            L.check(lib.codon_train_crops(*pool, P_(lut.data_ptr()), P_(t.data_ptr()), P_(y.data_ptr()), st), "train_crops")
        if degrade_holes:
            L.check(lib.codon_bicubic_downsample_masked(B, crop, scale, P_(src.data_ptr()), P_(wdown.data_ptr()),
                                                        P_(tab.data_ptr()), top, P_(lr.data_ptr()), st),
                    "bicubic_downsample_masked")
        else:
            L.check(lib.codon_bicubic_downsample(B, crop, scale, P_(src.data_ptr()), P_(wdown.data_ptr()), P_(lr.data_ptr()),
                                                 st), "bicubic_downsample")
        noisy = lr                                      # what the up launch reads
        if sensor is not None:
            noisy = torch.empty_like(lr)
            sd = L.SensorDesc()
            sd.batch, sd.size, sd.masked = B, p, 1 if degrade_holes else 0
            sd.seed_lo, sd.seed_hi = sensor.seed & 0xFFFFFFFF, sensor.seed >> 32
            sd.step, sd.first_sample = step, first_sample
            sd.sigma, sd.quad, sd.edge_thr = (np.float32(np.float64(c) / top) for c in
                                              (sensor.noise, sensor.noise_quad, sensor.edge_threshold))
            sd.p_drop, sd.p_edge = sensor.dropout, sensor.edge_dropout
            gauss = on_device("gauss", gauss_table, dev)
            L.check(lib.codon_lr_sensor(C.byref(sd), P_(lr.data_ptr()), P_(gauss.data_ptr()), P_(tab.data_ptr()), top,
                                        P_(noisy.data_ptr()), st), "lr_sensor")
        if fill_holes:                                  # degrade_holes: refused otherwise
            filled = torch.empty_like(noisy)
            _fill_launch(dev, B, p, p, noisy.data_ptr(), L.FILL_F32, tab, top, filled.data_ptr())
            noisy = filled
        if degrade_holes:
            L.check(lib.codon_bicubic_upsample_masked(B, p, p, scale, P_(noisy.data_ptr()), P_(wup.data_ptr()),
                                                      P_(x.data_ptr()), None, st), "bicubic_upsample_masked")
        else:
            L.check(lib.codon_bicubic_upsample(B, p, p, scale, P_(noisy.data_ptr()), P_(wup.data_ptr()), P_(x.data_ptr()), st),
                    "bicubic_upsample")
        if deep:
            L.check(lib.codon_quantize_levels(x.numel(), P_(x.data_ptr()), P_(tab.data_ptr()), top, st), "quantize_levels")
        else:
            L.check(lib.codon_quantize_u8(x.numel(), P_(x.data_ptr()), P_(tab.data_ptr()), st), "quantize_u8")
    return (x, y, t, noisy) if return_lr else (x, y, t)


# ---- training -----------------------------------------------------------------------------------------------------------------

def _world(group):
    import torch.distributed as dist
    if not dist.is_initialized():
        return 0, 1
    return dist.get_rank(group), dist.get_world_size(group)


def lr_at(step: int, *, lr: float, schedule: str = "constant", warmup: int = 0, lr_min: float = 0.0, lr_steps: int = None) -> float:
    """The learning rate of step 1, 2, ...: a pure function of the step number (float64 on the host), so a resumed run needs
    nothing but the step.  Either schedule with warmup > 0: lr * step / warmup up to step `warmup`.  constant: lr.  cosine:
    from lr at step `warmup` down half a cosine to lr_min at step lr_steps, lr_min beyond.  lr_steps is the length of the
    CURVE, not of one invocation."""
    if schedule not in LR_SCHEDULES:
        raise ValueError(f"lr_at: schedule {schedule!r} ({', '.join(LR_SCHEDULES)})")
    lr, lr_min = float(lr), float(lr_min)
    if warmup > 0 and step <= warmup:
        return lr * step / warmup
    if schedule == "constant":
        return lr
    if lr_steps is None or lr_steps <= warmup:
        raise ValueError(f"lr_at: the cosine curve needs lr_steps > warmup (lr_steps {lr_steps}, warmup {warmup})")
    if step > lr_steps:
        return lr_min
    return lr_min + (lr - lr_min) * 0.5 * (1.0 + math.cos(math.pi * (step - warmup) / (lr_steps - warmup)))


def save_checkpoint(path: str, step: int, model, opt, rng: np.random.Generator, args: dict):
    """Atomically (tmp file, then os.replace): a reader never sees half a checkpoint."""
    ck = {"epoch": int(step), "model": {k: v.detach().cpu() for k, v in model.state_dict().items()},
          "optimizer": opt.state_dict(), "rng": rng.bit_generator.state, "args": dict(args)}
    if opt.ema is not None:
        ck["model_ema"] = opt.ema_state_dict(model)
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    tmp = f"{path}.tmp{os.getpid()}"
    torch.save(ck, tmp)
    os.replace(tmp, path)


def load_resume(path: str, args: dict) -> dict:
    """A checkpoint written by save_checkpoint, refused if it was trained with another scale, crop, batch or dtype, or with
    other options that change the trajectory (RESUME_ALL_KEYS; a key the checkpoint's args lack compares as its default in
    RESUME_ALL_DEFAULTS)."""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(ck, dict) or not all(k in ck for k in ("epoch", "model", "optimizer", "rng", "args")):
        raise ValueError(f"--resume {path}: not a codon_amd.train checkpoint (use --weights to start from other weights)")
    was, now = ({k: a.get(k, RESUME_ALL_DEFAULTS.get(k)) for k in RESUME_ALL_KEYS} for a in (ck["args"], args))
    bad = [f"{k} {was[k]!r} != {now[k]!r}" for k in RESUME_ALL_KEYS if was[k] != now[k]]
    if bad:
        raise ValueError(f"--resume {path}: the checkpoint was trained with other arguments: {', '.join(bad)}")
    return ck


def fit(model, trainset: TrainSet, steps: int, *, scale: int, crop: int = 128, batch: int = 16, lr: float = 1e-4,
        dtype: str = "bf16", rng: np.random.Generator = None, seed: int = 0, log_every: int = 10, process_group=None,
        val: dict = None, ckpt: dict = None, start_step: int = 0, opt_state: dict = None, fixed: np.ndarray = None,
        args: dict = None, time_synth: bool = False, emit=print, clip_norm: float = None, skip_nonfinite: bool = False,
        ema_decay: float = None, lr_schedule: str = "constant", warmup: int = 0, lr_min: float = 0.0, lr_steps: int = None,
        grad_hook=None, mask_holes: bool = False, min_valid: float = 0.0, degrade_holes: bool = False,
        sensor: SensorModel = None, fill_holes: bool = False, normalize: bool = False, fill_guided: bool = False,
        fill_sigma: float = FILL_SIGMA) -> dict:
    """Train `model` (fp32 parameters on the pool's device) from step start_step + 1 to step `steps`.
    val:   {"depth", "color", "label", "every"} -- rank 0 runs infer.run_loop every `every` steps and prints the means;
    ckpt:  {"path", "every"} -- rank 0 saves every `every` steps and after the last one; a checkpoint's args are `args` with
           the run's trajectory options (options.RunOptions.of_fit of the arguments below and the TrainSet) laid over them;
    fixed: descriptors (draw's rows of this rank) used for EVERY step instead of drawing (overfit checks);
    time_synth: HIP events around synthesize and around each whole step (result["synth_ms"], ["step_ms"]);
    clip_norm, skip_nonfinite, ema_decay: FlatAdam's max_norm, skip_nonfinite, ema_decay (all off by default); with one on,
           the log lines gain `gnorm .. skipped N clipped N` and the result "stats" (FlatAdam.stats());
    lr_schedule, warmup, lr_min, lr_steps: lr_at's curve (lr_steps defaults to `steps`); with the constant schedule and no
           warm-up no learning rate is passed to the optimizer, so the one a resumed optimizer state carries rules;
    grad_hook(step, gs): called between gs.backward and gs.all_reduce_grads (gradient noise, freezing a tensor, tests).
    mask_holes: the criterion is MaskedL1SSIMLoss with valid = (t != 0) -- holes of the target (the label plane if the
           TrainSet has one) carry no loss and no gradient; the log lines gain ` valid 0.xxx`, the global batch's
           valid fraction, computed on the host from the descriptors (no device read);
    min_valid: draw's threshold (needs mask_holes).
    degrade_holes: synthesize's hole-aware degradation; needs no other option.
    A TrainSet with low-resolution maps (lr_dir) needs no argument here: synthesize reads the real maps, and the
           checkpoint's args gain train_lr_depth=True.
    sensor: synthesize's sensor model, given the step number and this rank's shard start -- also under `fixed`
           descriptors, so N ranks see the global batch one process sees and a resumed run the maps the straight run saw; the
           checkpoint's args gain the model's fields (SENSOR_DEFAULTS' keys).
    fill_holes, fill_guided, fill_sigma, normalize: the preparation of the low-resolution maps (prep.LrPrep's fields, DESIGN
           12.12).  A TrainSet of low-resolution maps is prepared once, when it is built, so fit and the TrainSet must agree on
           every one of them (either way round is refused); fill_holes alone also goes with degrade_holes on the synthetic path
           (synthesize's hole filling).  The checkpoint's args gain the options that are set, and a `val` dict with
           "lr_depth" and the same keys validates as `infer --lr-depth` with the same flags does.
    Returns {"losses": [(step, loss)], "gs", "opt", "rng", "step", ...}."""
    from .dist import FlatAdam, GradSync
    from .metrics import L1SSIMLoss, MaskedL1SSIMLoss
    if dtype not in DTYPES:
        raise ValueError(f"fit: dtype {dtype!r} (training runs in {', '.join(DTYPES)}; fp16 is inference-only)")
    rank, world = _world(process_group)
    if batch % world:
        raise ValueError(f"fit: a batch of {batch} does not split evenly over {world} ranks")
    check_min_valid("fit", min_valid, mask_holes)
    if lr_schedule == "cosine" and lr_steps is None:
        lr_steps = steps
    options = RunOptions.of_fit(trainset, locals())     # the keyword arguments above, by name: what the checkpoints will hold
    prep, built = options.prep, trainset.prep
    if trainset.has_lr and prep.fill_holes != built.fill_holes:
        raise ValueError("fit: fill_holes needs degrade_holes, or a TrainSet of low-resolution maps -- and that TrainSet must "
                         "have been built with the same fill_holes (its pool is filled once, when it is built)")
    check_fill("fit", trainset, prep.fill_holes, degrade_holes)
    if (prep.fill_guided, prep.fill_sigma) != (built.fill_guided, built.fill_sigma):
        say = lambda p: f"fill_guided {p.fill_guided!r}" + (f" (fill_sigma {p.fill_sigma!r})" if p.fill_guided else "")   # noqa: E731
        raise ValueError(f"fit: {say(prep)} with a TrainSet built with {say(built)}"
                         " -- only a TrainSet of low-resolution maps is filled with guidance, once, when it is built")
    if prep.normalize != built.normalize:
        raise ValueError(f"fit: normalize {prep.normalize!r} with a TrainSet built with normalize {built.normalize!r} (its "
                         "pool is stretched once, when it is built)")
    synth_kw = {"fill_holes": True} if prep.fill_holes else {}      # without it synthesize is called as ever
    if sensor is not None:                          # refused before the first step; without a model synthesize is called as ever
        from .dist import shard_batch
        check_sensor("fit", trainset, sensor, degrade_holes)
        synth_kw.update(sensor=sensor, first_sample=shard_batch(batch, rank, world)[0])
    rng = np.random.default_rng(seed) if rng is None else rng
    dev = trainset.pool.device
    model.set_compute_dtype(DTYPES[dtype])
    model.train()
    gs = GradSync(model, process_group=process_group)
    gs.broadcast_parameters(0)
    opt = FlatAdam(gs, lr=lr, max_norm=clip_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay)
    if opt_state is not None:
        opt.load_state_dict(opt_state)
    scheduled = lr_schedule != "constant" or warmup > 0
    lr_at(1, lr=lr, schedule=lr_schedule, warmup=warmup, lr_min=lr_min, lr_steps=lr_steps)       # refuses a bad curve up front
    crit = MaskedL1SSIMLoss(1.0, 1.0) if mask_holes else L1SSIMLoss(1.0, 1.0)
    if mask_holes:
        trainset.valid_integrals()                  # the one read of the pool, before the first step
    args = {**(args or {}), **options.args()}       # keys the table does not know (lr, seed) pass through
    stream = torch.cuda.current_stream(dev)
    losses, val_log, ev = [], [], []
    t_log, s_log = time.perf_counter(), start_step
    step = start_step
    for step in range(start_step + 1, steps + 1):
        if fixed is not None:
            descs = all_descs = fixed
        elif mask_holes:
            from .dist import shard_batch
            all_descs = draw(rng, trainset, batch, crop, min_valid=min_valid)      # the whole batch, as every rank draws it
            lo, hi = shard_batch(batch, rank, world)
            descs = all_descs[lo:hi]
        else:
            descs = draw(rng, trainset, batch, crop, rank, world)
        if time_synth:
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record(stream)
        gs.zero_grad()
        if time_synth:
            e[1].record(stream)
        if sensor is not None:
            synth_kw["step"] = step
        x, y, t = synthesize(trainset, descs, scale, crop, degrade_holes=degrade_holes, **synth_kw)
        if time_synth:
            e[2].record(stream)
        out = model(x, y)
        loss = crit(out.float(), t)
        gs.backward(loss)
        if grad_hook is not None:
            grad_hook(step, gs)
        gs.all_reduce_grads()
        if scheduled:
            opt.step(lr_at(step, lr=lr, schedule=lr_schedule, warmup=warmup, lr_min=lr_min, lr_steps=lr_steps))
        else:
            opt.step()
        if time_synth:
            e[3].record(stream)
            ev.append(e)
        if step % log_every == 0 or step == steps:
            lv = loss.detach().double().reshape(1)
            if world > 1:
                import torch.distributed as dist
                if dist.get_backend(process_group) == "gloo":
                    lv = lv.cpu()
                dist.all_reduce(lv, op=dist.ReduceOp.SUM, group=process_group)
                lv = lv / world                     # equal shards: the mean of the shard losses is the batch loss
            lv = float(lv.item())
            now = time.perf_counter()
            sps = (step - s_log) / (now - t_log)
            t_log, s_log = now, step
            losses.append((step, lv))
            line = f"step {step} loss {lv:.6f} steps/s {sps:.2f} images/s {sps * batch:.1f}"
            if opt.guarded:                         # the loss read-back has synchronised already
                st = opt.stats()
                line += f" gnorm {st['norm']:.6g} skipped {st['skipped']} clipped {st['clipped']}"
            if mask_holes:
                line += f" valid {valid_counts(trainset, all_descs, crop).sum() / (len(all_descs) * crop * crop):.3f}"
            if rank == 0:
                emit(line)
        if val and rank == 0 and step % val["every"] == 0:
            val_log.append((step, validate(model, dev, val, emit)))
            t_log = time.perf_counter()             # validation time is not training time
        if ckpt and rank == 0 and (step % ckpt["every"] == 0 or step == steps):
            save_checkpoint(ckpt["path"], step, model, opt, rng, args)
    res = {"losses": losses, "val": val_log, "gs": gs, "opt": opt, "rng": rng, "step": step, "rank": rank, "world": world}
    if opt.guarded:
        res["stats"] = opt.stats()
    if time_synth and ev:
        torch.cuda.synchronize(dev)
        res["synth_ms"] = [e[1].elapsed_time(e[2]) for e in ev]
        res["step_ms"] = [e[0].elapsed_time(e[3]) for e in ev]
    return res


def validate(model, dev, val: dict, emit=print) -> dict:
    """infer.run_loop over the validation set in eval mode at the training compute dtype; prints the mean masked RMSE and
    SSIM (the numbers the reference's test.py prints), then returns the model to train().  val["depth_bits"] == 16: the set
    is read as 16-bit with val["depth_max"], and the RMSE is in codes."""
    model.eval()
    try:
        with torch.no_grad():
            deep = {"depth_bits": 16, "depth_max": val.get("depth_max", 65535)} if val.get("depth_bits", 8) == 16 else {}
            if val.get("lr_depth"):                 # low-resolution validation maps, upsampled as infer --lr-depth does
                deep.update(lr_depth=val["lr_depth"], scale=val["scale"])
                deep.update(LrPrep.from_mapping(val).set_options())       # prepared as infer --lr-depth prepares them
            if val.get("report") is not None:       # the evaluation suite of infer --report
                deep.update(report=val["report"])
            r = run_loop(model, dev, torch.float32, val.get("depth"), val["color"], val.get("label"), emit=lambda s: None, **deep)
    finally:
        model.train()
    emit(f"val {r['n']} images rmse {r['rmse_mean']} ssim {r['ssim_mean']}")
    if val.get("report") is not None:
        emit("val-report " + report_tokens(r["report_means"]))
    return r


# ---- the command line ---------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, required=True, choices=[4, 8, 16])
    ap.add_argument("--train-depth", required=True, help="HR depth maps (PNG, 8-bit; 16-bit with --depth-bits 16)")
    ap.add_argument("--train-color", required=True, help="guidance images, paired with the depth maps by file name")
    ap.add_argument("--train-label", default=None,
                    help="targets, paired by file name: the depth maps are then only degraded into inputs (hole-filled depth "
                         "with holey labels, as the reference's data)")
    ap.add_argument("--train-lr-depth", default=None,
                    help="real low-resolution depth maps (codes, 0 a hole), paired by file name and --scale times smaller than "
                         "the pairs they fix the size of: the inputs are built from them as `codon_amd.infer --lr-depth` "
                         "builds its own, and --train-depth is the target (no synthetic degradation)")
    ap.add_argument("--mask-holes", action="store_true",
                    help="pixels whose target is 0 carry no loss and no gradient (the rule of the printed RMSE)")
    ap.add_argument("--min-valid", type=float, default=0.0,
                    help="with --mask-holes: redraw a crop with less than this fraction of valid pixels")
    ap.add_argument("--depth-bits", type=int, default=8, choices=[8, 16],
                    help="16: depth maps and labels (training and validation) are 16-bit PNGs of codes 0 .. --depth-max, 0 a "
                         "hole, value = code / depth-max; guidance stays 8-bit")
    ap.add_argument("--depth-max", type=int, default=None, help="with --depth-bits 16: the code of 1.0 (default 65535)")
    ap.add_argument("--crop", type=int, default=128)
    ap.add_argument("--batch", type=int, default=16, help="global batch (split over the ranks under torchrun)")
    ap.add_argument("--steps", type=int, default=1000, help="total steps (a resumed run continues up to this step)")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "f16"], help="f16 is refused: inference-only")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--save", default=None)
    ap.add_argument("--save-every", type=int, default=1000)
    ap.add_argument("--resume", default=None,
                    help="a checkpoint of this script: model, optimizer (its lr included) and generator state")
    ap.add_argument("--weights", default=None, help="initial weights: any checkpoint io.load_checkpoint reads")
    ap.add_argument("--degrade-holes", action="store_true",
                    help="holes (code 0) of the depth maps are left out of the degradation's two bicubics instead of being "
                         "smeared through them; the low-resolution map keeps them as holes, as a sensor's file does")
    add_prep_args(ap, {
        "fill_holes": "fill the holes of the low-resolution maps on the device by pull-push before they are upsampled, as "
                      "`codon_amd.infer --lr-depth --fill-holes` does: the maps of --train-lr-depth (once, when they are "
                      "loaded) or the synthetic ones of --degrade-holes (every step), and those of --val-lr-depth",
        "fill_guided": "with --train-lr-depth --fill-holes: guidance-aware filling, as `codon_amd.infer --lr-depth --fill-holes "
                       "--fill-guided` does it -- every record's low-resolution map is filled once, when the data is loaded, "
                       "with the record's own guidance plane deciding which side of an edge a hole is filled from (DESIGN "
                       "12.11); also applies to --val-lr-depth.  Refused with --degrade-holes",
        "normalize": "per-image range normalisation, as `codon_amd.infer --lr-depth --normalize` does it: when the data is "
                     "loaded, the valid codes [lo, hi] of every map are stretched onto [1, top] of the code grid on the "
                     "device, holes staying holes -- the low-resolution map of --train-lr-depth by its own range (after "
                     "--fill-holes) and its HR target by the same range, else the depth map by its own; also applies to "
                     "--val-lr-depth; refused with --train-label"})
    ap.add_argument("--sensor-noise", type=float, default=None, metavar="CODES",
                    help="sensor model: Gaussian noise of this standard deviation, in codes of the data's grid (255, or "
                         "--depth-max), on the synthetic low-resolution map; every --sensor option draws from --seed")
    ap.add_argument("--sensor-noise-quad", type=float, default=None, metavar="CODES",
                    help="sensor model: noise that grows with the square of the value v (0..1): CODES * v^2 more codes")
    ap.add_argument("--sensor-dropout", type=float, default=None, metavar="P",
                    help="sensor model: a valid low-resolution pixel becomes a hole with this probability (needs --degrade-holes)")
    ap.add_argument("--sensor-edge-dropout", type=float, default=None, metavar="P",
                    help="sensor model: this much more dropout where a 4-neighbour differs by more than "
                         "--sensor-edge-threshold (needs --degrade-holes)")
    ap.add_argument("--sensor-edge-threshold", type=float, default=None, metavar="CODES",
                    help="with --sensor-edge-dropout: the difference to a neighbour, in codes, above which a pixel is on an edge")
    ap.add_argument("--val-depth", default=None)
    ap.add_argument("--val-lr-depth", default=None,
                    help="low-resolution validation depth maps, upsampled by --scale as `codon_amd.infer --lr-depth` does "
                         "(instead of --val-depth)")
    ap.add_argument("--val-color", default=None)
    ap.add_argument("--val-label", default=None)
    ap.add_argument("--val-every", type=int, default=1000)
    ap.add_argument("--val-report", action="store_true",
                    help="with --val-label: a second line per validation, `val-report ...`, with the means of the evaluation "
                         "suite of `codon_amd.infer --report` over the validation set")
    add_report_args(ap, "val-")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--clip-norm", type=float, default=None, help="clip the global gradient norm to this (on the device)")
    ap.add_argument("--skip-nonfinite", action="store_true",
                    help="a step whose gradient holds an Inf or NaN changes nothing (it still counts as a step)")
    ap.add_argument("--ema", type=float, default=None,
                    help="keep EMA weights with this decay: saved as \"model_ema\", read by `codon_amd.infer --ema`")
    ap.add_argument("--lr-schedule", default="constant", choices=list(LR_SCHEDULES))
    ap.add_argument("--warmup-steps", type=int, default=0, help="linear warm-up from lr / N to lr over the first N steps")
    ap.add_argument("--lr-min", type=float, default=None, help="cosine: the learning rate at and after --lr-steps (default 0)")
    ap.add_argument("--lr-steps", type=int, default=None,
                    help="cosine: the length of the curve (default --steps); give it when a run is cut into --resume legs")
    a = ap.parse_args(argv)
    if a.dtype == "f16":
        ap.error("--dtype f16: fp16 training is not supported (inference-only, as in the reference); use bf16 or f32")
    if a.crop % a.scale or a.crop // a.scale < 4:
        ap.error(f"--crop {a.crop} must be a multiple of --scale {a.scale} and at least 4 * scale")
    if a.batch < 1 or a.steps < 1 or a.log_every < 1 or a.save_every < 1 or a.val_every < 1:
        ap.error("--batch, --steps, --log-every, --save-every and --val-every must be positive")
    if a.resume and a.weights:
        ap.error("--resume and --weights exclude each other")
    if a.val_depth is not None and a.val_lr_depth is not None:
        ap.error("--val-depth and --val-lr-depth exclude each other")
    if (a.val_depth is None and a.val_lr_depth is None) != (a.val_color is None):
        ap.error("--val-depth (or --val-lr-depth) and --val-color go together")
    if a.val_report and a.val_label is None:
        ap.error("--val-report needs --val-label")
    if not a.val_report:
        for n in ("val_bad_thresholds", "val_edge_threshold", "val_edge_radius"):
            if getattr(a, n) is not None:
                ap.error(f"--{n.replace('_', '-')} needs --val-report")
    a.val_report_params = report_of(ap, a, "val-") if a.val_report else None
    if a.train_lr_depth is not None and a.train_label is not None:
        ap.error("--train-lr-depth and --train-label exclude each other (with low-resolution maps --train-depth is the target)")
    if a.train_lr_depth is not None and a.degrade_holes:
        ap.error("--train-lr-depth and --degrade-holes exclude each other (nothing is degraded)")
    if a.fill_holes and a.train_lr_depth is None and not a.degrade_holes:
        ap.error("--fill-holes needs --train-lr-depth or --degrade-holes (the unmasked degradation has no holes to fill)")
    if a.fill_guided and a.degrade_holes:
        ap.error("--fill-guided is refused with --degrade-holes: the synthetic path holds its guidance as fp32 D4 crops, not as "
                 "the codes of a whole image (only the real maps of --train-lr-depth and --val-lr-depth are filled with guidance)")
    a.prep = prep_of(ap, a, a.fill_holes and a.train_lr_depth is not None, "--train-lr-depth --fill-holes")
    if a.normalize and a.train_label is not None:
        ap.error("--normalize and --train-label exclude each other (a label plane has no range of its own to be stretched by)")
    given = {n: getattr(a, "sensor_" + n) for n in ("noise", "noise_quad", "dropout", "edge_dropout", "edge_threshold")}
    given = {n: v for n, v in given.items() if v is not None}
    if given:
        opt = lambda n: "--sensor-" + n.replace("_", "-")                  # noqa: E731
        if a.train_lr_depth is not None:
            ap.error(f"{opt(next(iter(given)))} and --train-lr-depth exclude each other (nothing is degraded: real "
                     "low-resolution maps carry their sensor's own noise and holes)")
        for n in ("dropout", "edge_dropout"):
            if n in given and not a.degrade_holes:
                ap.error(f"{opt(n)} needs --degrade-holes (a dropped pixel must be left out of the upsample)")
        if ("edge_dropout" in given) != ("edge_threshold" in given):
            ap.error("--sensor-edge-dropout and --sensor-edge-threshold go together")
        for n, v in given.items():
            if not math.isfinite(v) or v < 0:
                ap.error(f"{opt(n)} {v} must be finite and not negative")
        if max(given.get("dropout", 0.0), given.get("edge_dropout", 0.0)) > 1 or \
                given.get("dropout", 0.0) + given.get("edge_dropout", 0.0) > 1:
            ap.error("--sensor-dropout and --sensor-edge-dropout are probabilities, together at most 1")
        if a.crop // a.scale > 512:
            ap.error(f"the sensor model takes low-resolution maps up to 512 (--crop {a.crop} at x{a.scale})")
        if not 0 <= a.seed < 1 << 64:
            ap.error(f"--seed {a.seed} must lie in [0, 2^64) with a sensor model")
    if a.degrade_holes and a.crop > 1024:
        ap.error(f"--degrade-holes takes crops up to 1024 (--crop {a.crop})")
    if not 0.0 <= a.min_valid <= 1.0:
        ap.error(f"--min-valid {a.min_valid} must lie in [0, 1]")
    if a.min_valid > 0 and not a.mask_holes:
        ap.error("--min-valid needs --mask-holes")
    if a.depth_max is not None and a.depth_bits != 16:
        ap.error("--depth-max belongs to --depth-bits 16")
    a.depth_max = 65535 if a.depth_max is None else a.depth_max
    if not 1 <= a.depth_max <= 65535:
        ap.error(f"--depth-max {a.depth_max} must lie in [1, 65535]")
    if a.clip_norm is not None and not a.clip_norm > 0:
        ap.error(f"--clip-norm {a.clip_norm} must be positive")
    if a.ema is not None and not 0 <= a.ema < 1:
        ap.error(f"--ema {a.ema} must lie in [0, 1)")
    if a.lr_schedule == "constant" and (a.lr_min is not None or a.lr_steps is not None):
        ap.error("--lr-min and --lr-steps belong to --lr-schedule cosine")
    if a.lr_steps is not None and a.lr_steps < 1:
        ap.error(f"--lr-steps {a.lr_steps} must be positive")
    if a.lr_min is not None and not 0 <= a.lr_min <= a.lr:
        ap.error(f"--lr-min {a.lr_min} must lie in [0, --lr {a.lr}]")
    if a.lr_schedule == "cosine":
        a.lr_steps = a.steps if a.lr_steps is None else a.lr_steps       # resolved: the curve's length, not this invocation's
    a.lr_min = 0.0 if a.lr_min is None else a.lr_min
    curve = a.lr_steps if a.lr_steps is not None else a.steps
    if a.warmup_steps < 0 or a.warmup_steps >= curve:
        ap.error(f"--warmup-steps {a.warmup_steps} must lie in [0, {curve}): shorter than the run's {curve} steps")
    return a


def main(argv=None, emit=print) -> dict:
    a = parse_args(argv)
    prep = a.prep
    args = run_args(a)
    resume = load_resume(a.resume, args) if a.resume else None     # refused before any GPU work
    import torch.distributed as dist
    group = None
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ and not dist.is_initialized():
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group(a.dist_backend)
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found, codon_amd has no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    rank, world = _world(group)
    if a.batch % world:
        raise SystemExit(f"--batch {a.batch} does not split evenly over {world} ranks")
    if a.batch // world > L.TRAIN_MAX_BATCH:
        raise SystemExit(f"--batch {a.batch}: at most {L.TRAIN_MAX_BATCH} images per rank")
    ts = TrainSet(a.train_depth, a.train_color, dev, crop=a.crop, label_dir=a.train_label, depth_bits=a.depth_bits,
                  depth_max=a.depth_max, **({"lr_dir": a.train_lr_depth, "scale": a.scale} if a.train_lr_depth else {}),
                  # the synthetic maps of --degrade-holes are filled every step, by synthesize: only real ones in the pool
                  **(prep if a.train_lr_depth else dataclasses.replace(prep, fill_holes=False)).set_options())
    torch.manual_seed(a.seed)
    model = (CODONNet16 if a.scale == 16 else CODONNet)()
    rng = np.random.default_rng(a.seed)
    start, opt_state = 0, None
    if resume is not None:
        model.load_state_dict(resume["model"], strict=True)
        rng.bit_generator.state = resume["rng"]
        start, opt_state = int(resume["epoch"]), resume["optimizer"]
        if rank == 0:
            emit(f"resumed {a.resume} at step {start}")
    elif a.weights:
        ep = io.load_checkpoint(a.weights, model)
        if rank == 0:
            emit(f"loaded {a.weights} (epoch {ep})")
    model = model.to(dev)
    if rank == 0:
        emit(f"{len(ts)} training pairs, x{a.scale}, crop {a.crop}, batch {a.batch} over {world} rank(s), {a.dtype}, "
             f"steps {start + 1}..{a.steps}")
    val = ({"depth": a.val_depth, "color": a.val_color, "label": a.val_label, "every": a.val_every,
            "depth_bits": a.depth_bits, "depth_max": a.depth_max} if a.val_depth or a.val_lr_depth else None)
    if a.val_lr_depth:
        val.update(lr_depth=a.val_lr_depth, scale=a.scale, **prep.set_options())
    if val is not None and a.val_report_params is not None:
        val.update(report=a.val_report_params)
    ckpt = {"path": a.save, "every": a.save_every} if a.save else None
    res = fit(model, ts, a.steps, rng=rng, process_group=group, val=val, ckpt=ckpt, start_step=start, opt_state=opt_state,
              args=args, emit=emit, **fit_kwargs(a))
    res["model"] = model
    return res


if __name__ == "__main__":
    main()
    import torch.distributed as _dist
    if _dist.is_initialized():
        _dist.destroy_process_group()
