"""Geometric self-ensemble at inference time (the "+" variant of super-resolution code bases): the network runs on
the eight flips and rotations of its input -- the D4 operations codon_amd.train augments with -- each output is flipped and
rotated back, and the eight are averaged.  Both data movements are ONE launch each of a hand-written kernel (csrc/d4.hip):
codon_d4_views builds all eight views of depth and guidance, codon_d4_merge forms the mean.  Defined bit for bit in
tests/d4_ref.py."""
import ctypes as C

import torch

from . import _lib as L
from . import ops

_P = C.c_void_p


def d4_views(x: torch.Tensor, y: torch.Tensor = None):
    """(upright_x, transposed_x[, upright_y, transposed_y]): the eight D4 views of every (H,W) plane of x (B,1,H,W) -- and of y,
    in the same launch -- as an upright batch (4B,1,H,W) of codes 0, 2, 4, 6 and a transposed batch (4B,1,W,H) of codes 1, 3, 5,
    7; view k of image b is image 4*b + (k >> 1) of its batch.  Bits are copied, nothing is computed."""
    dev = ops._dev(x, y)
    if x.dim() != 4 or x.shape[1] != 1 or x.dtype not in ops.DTYPE_CODE or (y is not None and (y.shape != x.shape or y.dtype != x.dtype)):
        raise RuntimeError("d4_views expects (B,1,H,W) planes of one shape and one dtype (fp32, fp16 or bf16)")
    B, _, H, W = x.shape
    outs = [torch.empty((4 * B, 1) + hw, dtype=x.dtype, device=dev) for _ in ((x,) if y is None else (x, y)) for hw in ((H, W), (W, H))]
    ptrs = [_P(t.data_ptr()) for t in outs] + [None, None]
    with ops._on(dev):
        L.check(L.load().codon_d4_views(B, H, W, _P(x.data_ptr()), _P(y.data_ptr()) if y is not None else None, ops.DTYPE_CODE[x.dtype],
                                        ptrs[0], ptrs[1], ptrs[2], ptrs[3], ops._stream(dev)), "d4_views")
    return tuple(outs)


def d4_merge(upright: torch.Tensor, transposed: torch.Tensor) -> torch.Tensor:
    """fp32 (B,1,H,W): 0.125f * (((u0+u1)+(u2+u3)) + ((u4+u5)+(u6+u7))), u_k the inverse of view k taken from the network's
    outputs on d4_views' two batches, upcast exactly to fp32 -- whatever their dtype, the mean is fp32."""
    dev = ops._dev(upright, transposed)
    n = upright.shape[0] if upright.dim() == 4 else -1
    if (n < 0 or n % 4 or upright.shape[1] != 1 or transposed.shape != (n, 1, upright.shape[3], upright.shape[2])
            or upright.dtype not in ops.DTYPE_CODE or transposed.dtype != upright.dtype):
        raise RuntimeError(f"d4_merge expects (4B,1,H,W) and (4B,1,W,H) of one dtype (fp32, fp16 or bf16), got "
                           f"{tuple(upright.shape)} {upright.dtype} and {tuple(transposed.shape)} {transposed.dtype}")
    _, _, H, W = upright.shape
    out = torch.empty((n // 4, 1, H, W), dtype=torch.float32, device=dev)
    with ops._on(dev):
        L.check(L.load().codon_d4_merge(n // 4, H, W, _P(upright.data_ptr()), _P(transposed.data_ptr()), ops.DTYPE_CODE[upright.dtype],
                                        _P(out.data_ptr()), ops._stream(dev)), "d4_merge")
    return out


def self_ensemble(model, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The mean over the eight D4 views of model's output, as fp32 (B,1,H,W) -- ALWAYS fp32: the mean of eight 16-bit values
    needs the extra bits.  x: HR-sized depth, y: guidance, (B,1,H,W) on the GPU, one dtype (fp32, fp16 or bf16).

    model: any callable taking and returning (N,1,h,w) tensors (a CODONNet in eval mode, or a stand-in).  It is called exactly
    TWICE, on 4B views each: model(upright_x, upright_y) at (4B,1,H,W) and model(transposed_x, transposed_y) at (4B,1,W,H) --
    square images included, where one call on 8B views would do: one rule means one launch schedule per image shape.

    One codon_d4_views launch, the two forwards, one codon_d4_merge launch, all on the caller's current stream, under
    torch.no_grad(), with no host synchronisation."""
    if x.shape != y.shape or x.dim() != 4 or x.shape[1] != 1:
        raise RuntimeError(f"self_ensemble expects two (B,1,H,W) tensors, got {tuple(x.shape)} and {tuple(y.shape)}")
    if not (x.is_cuda and y.is_cuda):
        raise RuntimeError("self_ensemble runs on MI355X only: move the model and inputs to 'cuda' (there is no CPU fallback)")
    if x.dtype not in ops.DTYPE_CODE or y.dtype != x.dtype:
        raise NotImplementedError(f"self_ensemble: input dtypes {x.dtype} and {y.dtype} not supported (one of fp32, bf16, fp16 for both)")
    if getattr(model, "training", False):
        raise RuntimeError("self_ensemble is inference only: the model is in training mode, call .eval() first")
    B, _, H, W = x.shape
    if B == 0:
        return torch.zeros((0, 1, H, W), dtype=torch.float32, device=x.device)     # the C ABI itself refuses batch 0
    with torch.no_grad():
        ux, tx, uy, ty = d4_views(x.contiguous(), y.contiguous())
        ou, ot = model(ux, uy), model(tx, ty)
        for o, v in ((ou, ux), (ot, tx)):
            if not torch.is_tensor(o) or o.shape != v.shape:
                raise RuntimeError(f"self_ensemble: the model returned {tuple(o.shape) if torch.is_tensor(o) else type(o).__name__} "
                                   f"for views of shape {tuple(v.shape)}")
        return d4_merge(ou.contiguous(), ot.contiguous())
