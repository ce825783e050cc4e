"""Either side of the network in the reference's script, on device:
  postprocess_u8  clip -> *255 -> truncating uint8          /root/reference/CODON_X4/test.py:127-132
  masked_rmse     RMSE over label != 0, exact integer sums   /root/reference/CODON_X4/test.py:148-164
  postprocess_u16, masked_rmse_u16   their 16-bit counterparts: definitions of this project, no reference
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
