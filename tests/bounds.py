"""Per-element bounds for the MFMA conv kernels (test infrastructure, CPU only).

A conv kernel's output element is E(a): the fp32 accumulator a of the conv over the operands AS THE KERNEL SEES THEM
(already rounded to the tensor dtype), passed through the epilogue E (ReLU, + residual, mask, + prior contents) and, for
the 16-bit dtypes, rounded once to nearest even on the store.  With ref = the same conv in float64, S = |x| (*) |w| and

    tau = 2^-20 (S + |additive operands|)          (16 fp32 units of the absolute-value sum)

every element must satisfy

    16-bit:  round16(E(ref - tau)) <= got <= round16(E(ref + tau))
    fp32  :  E(ref - tau) <= got <= E(ref + tau)

Every epilogue here is monotone in the accumulator, so this interval is exact: it holds for any accumulation error up to
tau, and for nothing else.  The fp32 MFMA chain measures at 1 - 3.5e-7 S against float64 for K <= 4096; the 16-bit MFMAs'
internal accumulation error is ASSUMED to fit the same tau.  tau is far inside a 16-bit half-ulp for almost every element,
so most elements have exactly one allowed value (the correctly rounded one); assert_rounded refuses to pass a check in
which fewer than half of them do."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from codon_amd import _lib as L

TAU_UNIT = 2.0 ** -20
INFORMATIVE_SHARE = 0.5

_BF16_MIN_EXP = -133      # subnormal spacing of bf16 (and fp32's exponent range)
_BF16_BITS = 8            # significant bits, the implicit one included
_BF16_OVERFLOW = 2.0 ** 128


def _is16(dtype) -> bool:
    return dtype in (torch.bfloat16, torch.float16)


def round16(x64, dtype) -> np.ndarray:
    """float64 values of the nearest bf16 / fp16 numbers to x64 (array-like): ties to even, ONE rounding from float64,
    subnormals kept, overflow to +-inf.  (torch's float64 -> 16-bit .to() goes through float32 and rounds twice.)"""
    x = np.asarray(x64, dtype=np.float64)
    if dtype == torch.float16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float64)        # numpy rounds float64 -> half directly
    assert dtype == torch.bfloat16, dtype
    _, e = np.frexp(x)                                            # |x| in [2^(e-1), 2^e)
    q = np.maximum(e - _BF16_BITS, _BF16_MIN_EXP)                 # exponent of the bf16 spacing at x
    with np.errstate(invalid="ignore"):
        r = np.ldexp(np.rint(np.ldexp(x, -q)), q)                 # power-of-two scalings are exact; rint ties to even
    return np.where(np.abs(r) >= _BF16_OVERFLOW, np.copysign(np.inf, x), r)


def ulp(x64, dtype) -> np.ndarray:
    """Spacing of `dtype` numbers at |x64| (the subnormal spacing below the normal range)."""
    bits, emin = {torch.bfloat16: (8, -133), torch.float16: (11, -24), torch.float32: (24, -149)}[dtype]
    x = np.asarray(x64, dtype=np.float64)
    _, e = np.frexp(x)
    return np.where(x == 0, np.ldexp(1.0, emin), np.ldexp(1.0, np.maximum(e - bits, emin)))


def conv_ref(x, w, k: int, pack: int = L.PACK_FWD):
    """(ref, S): the conv the kernel computes, in float64 on the CPU, and the same conv of absolute values.
    x: (B, Cin, H, W) and w: the OIHW weight given to codon_conv_pack_weight, both already rounded to the tensor dtype.
    PACK_FWD: conv2d(x, w); PACK_DGRAD: conv_transpose2d(x, w) -- dL/dx of the forward conv w for dL/dy = x
    (x then has w.shape[0] channels).  Stride 1, 'same' padding."""
    x64, w64 = x.detach().cpu().double(), w.detach().cpu().double()
    op = {L.PACK_FWD: F.conv2d, L.PACK_DGRAD: F.conv_transpose2d}[pack]
    return op(x64, w64, None, 1, k // 2), op(x64.abs(), w64.abs(), None, 1, k // 2)


def tau_of(S, *additive):
    """tau = 2^-20 (S + sum of |additive operands|): 16 fp32 units of everything the epilogue sums."""
    t = S.double().clone()
    for a in additive:
        t += a.detach().cpu().double().abs()
    return t * TAU_UNIT


def _np(t) -> np.ndarray:
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def assert_rounded(got, ref, tau, dtype, what: str, epi=None, S=None, show: int = 6) -> dict:
    """Check every element of the kernel output `got` (B, C, H, W) against the float64 accumulator reference `ref` (the
    same shape) within `tau` (a tensor of that shape, see tau_of), with the epilogue `epi` (a monotone elementwise map of
    float64 tensors, identity when None) applied to ref -+ tau before the store rounding of `dtype`.  A NaN in `got`
    fails (outputs are NaN-prefilled: an element never written shows up).  Prints one summary line -- max |got - E(ref)| / S
    (S defaults to tau / 2^-20) and, for 16-bit, the share of elements whose interval holds ONE value, which must be at
    least 50 %: a check that allows several values for most elements says nothing.  Returns the summary numbers."""
    epi = epi or (lambda a: a)
    ref, tau = ref.detach().cpu().double(), tau.detach().cpu().double()
    g = _np(got)
    assert g.shape == tuple(ref.shape) == tuple(tau.shape), (what, g.shape, tuple(ref.shape), tuple(tau.shape))
    e_ref = _np(epi(ref))
    lo, hi = _np(epi(ref - tau)), _np(epi(ref + tau))
    if _is16(dtype):
        lo, hi = round16(lo, dtype), round16(hi, dtype)
    ok = (g >= lo) & (g <= hi)                                    # False for NaN
    scale = _np(S) if S is not None else _np(tau) / TAU_UNIT
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(scale > 0, np.abs(g - e_ref) / scale, np.abs(g - e_ref))
    err = float(np.nanmax(rel)) if rel.size and not np.isnan(rel).all() else float("nan")
    share = float((lo == hi).mean()) if _is16(dtype) and g.size else None
    print(f"[bounds] {what}: {g.size} elements, max|got-ref|/S {err:.3e}"
          + (f", decided exactly {100 * share:.1f} %" if share is not None else ""))
    nbad = int((~ok).sum())
    if nbad:
        idx = np.argwhere(~ok)[:show]
        u = ulp(e_ref, dtype)
        at = lambda a, i: float(a[tuple(i)])
        lines = [f"  (b,c,h,w)={tuple(int(v) for v in i)}: got {at(g, i)!r} ref {at(e_ref, i)!r} allowed "
                 f"[{at(lo, i)!r}, {at(hi, i)!r}] error {(at(g, i) - at(e_ref, i)) / at(u, i):+.2f} ulp" for i in idx]
        raise AssertionError(f"{what}: {nbad} of {g.size} elements outside the correctly rounded interval "
                             f"(tau = 2^-20 (S + |additive|)); first {len(idx)}:\n" + "\n".join(lines))
    if share is not None:
        assert share >= INFORMATIVE_SHARE, (
            f"{what}: only {100 * share:.1f} % of the elements have a single allowed value (< {100 * INFORMATIVE_SHARE:.0f} %): "
            "tau is too wide for this check to mean anything")
    return {"max_err_over_S": err, "exact_share": share, "n": int(g.size)}
