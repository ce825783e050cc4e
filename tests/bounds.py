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
which fewer than half of them do.

The weight gradients (wgrad_*, assert_wgrad) are fp32 sums over K = B H W pixels that are stored without an epilogue:
|got - ref| <= 2^-20 S per element, S = sum |gy| |x|.  The mean product is S / K, so the bound sees ONE dropped or doubled
product of ordinary size only while K 2^-20 <= 1/4 (the mean product is then >= 4 tau): assert_wgrad refuses larger cases.
wgrad_bands mirrors the launchers' band plans, so that a test can state which plan it runs and place its probes on the
seams; wgrad_impulse_expect states the exact result for one-hot operands."""
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


def assert_rounded(got, ref, tau, dtype, what: str, epi=None, S=None, show: int = 6, where=None) -> dict:
    """Check every element of the kernel output `got` (B, C, H, W) against the float64 accumulator reference `ref` (the
    same shape) within `tau` (a tensor of that shape, see tau_of), with the epilogue `epi` (a monotone elementwise map of
    float64 tensors, identity when None) applied to ref -+ tau before the store rounding of `dtype`.  A NaN in `got`
    fails (outputs are NaN-prefilled: an element never written shows up).  Prints one summary line -- max |got - E(ref)| / S
    (S defaults to tau / 2^-20) and, for 16-bit, the share of elements whose interval holds ONE value, which must be at
    least 50 %: a check that allows several values for most elements says nothing.  `where` (optional): index tuple -> text
    appended to that element's line of a failure message (the tile it lies in).  Returns the summary numbers."""
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
                 f"[{at(lo, i)!r}, {at(hi, i)!r}] error {(at(g, i) - at(e_ref, i)) / at(u, i):+.2f} ulp"
                 + (f": {where(tuple(int(v) for v in i))}" if where else "") for i in idx]
        raise AssertionError(f"{what}: {nbad} of {g.size} elements outside the correctly rounded interval "
                             f"(tau = 2^-20 (S + |additive|)); first {len(idx)}:\n" + "\n".join(lines))
    if share is not None:
        assert share >= INFORMATIVE_SHARE, (
            f"{what}: only {100 * share:.1f} % of the elements have a single allowed value (< {100 * INFORMATIVE_SHARE:.0f} %): "
            "tau is too wide for this check to mean anything")
    return {"max_err_over_S": err, "exact_share": share, "n": int(g.size)}


# ---- weight gradients -------------------------------------------------------------------------------------------------

WGRAD_K_CAP = int(0.25 / TAU_UNIT)          # B H W <= 262144: the mean product S / K is at least 4 tau

# tile heights of the weight-gradient kernels (rows of gy per staged tile)
WGRAD_TH16 = {5: 10, 3: 6, 1: 4}            # conv_wgrad_c8.hip: CODON_WC8_TH5, CODON_WC8_TH3, WC8_TH
WGRAD_TH32 = 4                              # conv_wgrad_f32.hip: TH; the planner of both fp32 kernels counts 4-row tiles
WGRAD_TH32_T16 = {5: 4, 3: 4, 1: 2}         # conv_wgrad_f32_t16.hip: TH (2 rows for k = 1)
WGRAD_TW = 32                               # every kernel: 32-pixel tile columns


def wgrad_bands(dtype, k: int, cin: int, cout: int, B: int, H: int, W: int, aligned: bool = True) -> dict:
    """The band plan of codon_conv2d_wgrad, restated: wgrad16_plan (conv_wgrad_c8.hip) for the 16-bit dtypes, wgrad_plan
    (conv_wgrad_f32.hip) for fp32, and each kernel's own spread of tile rows over the bands.  `aligned`: fp32 slices start
    on 16 bytes (with W % 4 == 0 that selects the 16x16x4 kernel; otherwise the round-1 kernel runs on the SAME split).
    Returns kernel, th (tile height), nbands, nsplit and bands = [(first tile row, one past the last)] per band.  The tests
    compare nsplit with codon_conv_wgrad_workspace_bytes before they rely on any of it.
    A mirror kept in step by hand (the band edges place the probes and word the failure messages; no result depends on them):
    the planners are wgrad16_plan and wgrad_plan, the spreads the ty_begin / ty_end lines of conv_wgrad_c8.hip (wgrad_c8 kernel,
    j tiles / nbands), conv_wgrad_f32_t16.hip (the same spread over its own tile height) and conv_wgrad_f32.hip (band_tiles_y
    rows per band, the last band clipped)."""
    cdiv = lambda a, b: (a + b - 1) // b
    if _is16(dtype):
        th = WGRAD_TH16[k]
        blocks = (cout // 64) * (cin // {5: 32, 3: 64, 1: 128}[k])
        tiles = cdiv(H, th)
        nbands = min(max(cdiv(256, blocks * B), 1), tiles)                     # WGRAD16_TARGET_BLOCKS
        bands = [(j * tiles // nbands, (j + 1) * tiles // nbands) for j in range(nbands)]
        kernel = "c8"
    else:
        co_t, ci_t = {5: (1, 1), 3: (2, 1), 1: (2, 2)}[k]
        t16_shape = W % 4 == 0
        blocks = (cout // 64) * (cin // (128 if k == 1 else 32)) if t16_shape else (cout // (32 * co_t)) * (cin // (32 * ci_t))
        tiles4 = cdiv(H, WGRAD_TH32)
        want = min(max(cdiv(256 if t16_shape else 1024, blocks * B), 1), tiles4)
        per = cdiv(tiles4, want)
        nbands = cdiv(tiles4, per)
        if t16_shape and aligned:
            th, kernel = WGRAD_TH32_T16[k], "f32_t16"
            tiles = cdiv(H, th)
            bands = [(j * tiles // nbands, (j + 1) * tiles // nbands) for j in range(nbands)]
        else:
            th, kernel, tiles = WGRAD_TH32, "f32_r1", tiles4
            bands = [(j * per, min((j + 1) * per, tiles4)) for j in range(nbands)]
    assert bands[0][0] == 0 and bands[-1][1] == tiles and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
    return {"kernel": kernel, "th": th, "tiles": tiles, "nbands": nbands, "nsplit": B * nbands, "bands": bands,
            "rows_per_band": [e - b for b, e in bands], "H": H, "W": W}


def wgrad_where(plan: dict, h: int, w: int) -> str:
    """'band j, tile row t (rows a..b), tile column c' of pixel (h, w) under `plan`: for failure messages."""
    t = h // plan["th"]
    j = next(i for i, (b, e) in enumerate(plan["bands"]) if b <= t < e)
    return (f"band {j} of {plan['nbands']} (tile rows {plan['bands'][j][0]}..{plan['bands'][j][1] - 1}), tile row {t} "
            f"(rows {t * plan['th']}..{t * plan['th'] + plan['th'] - 1}), tile column {w // WGRAD_TW}")


def wgrad_probe_pixels(plan: dict, B: int, H: int, W: int, n: int) -> list:
    """Rounds of n probe pixels (b, h, w) each, together covering: the four corners; both sides of EVERY seam between tile
    rows (band seams and the seams inside a band alike: rows m th - 1 and m th); the first and last row and column of a
    tile; the ragged last row and column; the first, a middle and the last image.  Rows and columns are paired round-robin,
    every row and column of interest is used at least once; the last round is filled up from the start of the list."""
    th = plan["th"]
    seams = [m * th for m in range(1, plan["tiles"])]
    band_seams = [b * th for b, _ in plan["bands"][1:]]
    rows = [0, H - 1] + [r for s in band_seams for r in (s - 1, s)] + [r for s in seams if s not in band_seams for r in (s - 1, s)]
    rows = list(dict.fromkeys(r for r in rows if 0 <= r < H))
    last = (W - 1) // WGRAD_TW * WGRAD_TW
    cols = list(dict.fromkeys(c for c in (0, W - 1, WGRAD_TW - 1, WGRAD_TW, last - 1, last, W // 2) if 0 <= c < W))
    imgs = list(dict.fromkeys((0, B - 1, B // 2)))
    pix = [(0, 0, 0), (B - 1, 0, W - 1), (B // 2, H - 1, 0), (B - 1, H - 1, W - 1)]
    m = max(len(rows), len(cols))
    for i in range(m):
        pix.append((imgs[(i // 2) % len(imgs)], rows[i % len(rows)], cols[i % len(cols)]))
    i = 0
    while len(pix) % n:                    # fill the last round: the same rows against other columns and images
        pix.append((imgs[(i + 1) % len(imgs)], rows[i % len(rows)], cols[(i + 3) % len(cols)]))
        i += 1
    return [pix[j:j + n] for j in range(0, len(pix), n)]


def wgrad_one_hot(pix: list, B: int, H: int, W: int) -> torch.Tensor:
    """(B, len(pix), H, W) fp32: channel c is 1.0 at its pixel pix[c] = (b, h, w) and 0 elsewhere."""
    t = torch.zeros((B, len(pix), H, W))
    for c, (b, h, w) in enumerate(pix):
        t[b, c, h, w] = 1.0
    return t


def wgrad_impulse_expect(dense: torch.Tensor, pix: list, k: int, hot: str) -> torch.Tensor:
    """The exact weight gradient dW (cout, cin, k, k) when one operand is one-hot per channel (wgrad_one_hot(pix)):
        hot == "gy": dW[co][ci][dy][dx] = x [b_co, ci, h_co + dy - p, w_co + dx - p]      dense = x  (B, cin,  H, W)
        hot == "x" : dW[co][ci][dy][dx] = gy[b_ci, co, h_ci - dy + p, w_ci - dx + p]      dense = gy (B, cout, H, W)
    and +0 where that pixel lies outside the image.  A gather, no arithmetic: exact in the dtype of `dense`."""
    assert hot in ("gy", "x")
    B, Cd, H, W = dense.shape
    p, n = k // 2, len(pix)
    out = torch.zeros((n, Cd, k, k), dtype=dense.dtype)
    for c, (b, h, w) in enumerate(pix):
        for dy in range(k):
            for dx in range(k):
                hh, ww = (h + dy - p, w + dx - p) if hot == "gy" else (h - dy + p, w - dx + p)
                if 0 <= hh < H and 0 <= ww < W:
                    out[c, :, dy, dx] = dense[b, :, hh, ww]
    return out if hot == "gy" else out.transpose(0, 1).contiguous()


def wgrad_impulse_diff(got, exp, pix: list, k: int, hot: str, plan: dict, show: int = 6):
    """None when the one-hot result `got` equals `exp` (wgrad_impulse_expect) exactly, else a message that names the first
    wrong elements: (co, ci, tap), the gy pixel whose product it is, that pixel's band, tile row and tile column under
    `plan`, and what the value looks like (missing, doubled, or the value of which neighbouring tap)."""
    got, exp = got.detach().cpu().float(), exp.detach().cpu().float()
    assert got.shape == exp.shape, (tuple(got.shape), tuple(exp.shape))
    if torch.equal(got, exp):
        return None
    bad = (got != exp) | torch.isnan(got)
    p, lines = k // 2, []
    for co, ci, dy, dx in np.argwhere(bad.numpy())[:show]:
        b, h, w = pix[co if hot == "gy" else ci]
        gh, gw = (h, w) if hot == "gy" else (h - dy + p, w - dx + p)          # the gy pixel of this product
        xh, xw = gh + dy - p, gw + dx - p
        g, e = float(got[co, ci, dy, dx]), float(exp[co, ci, dy, dx])
        if g != g:
            kind = "never written"
        elif g == 0 and e != 0:
            kind = "product missing"
        elif e != 0 and g == 2 * e:
            kind = "product counted twice"
        else:
            same = (exp[co, ci] == g).nonzero() if hot == "gy" else (exp[co, :, dy, dx] == g).nonzero()
            kind = f"the value expected at {'tap' if hot == 'gy' else 'ci'} {tuple(int(v) for v in same[0])}" if len(same) else "matches no neighbour"
        where = wgrad_where(plan, gh, gw) if 0 <= gh < plan["H"] and 0 <= gw < plan["W"] else "outside the image"
        lines.append(f"  (co,ci)=({co}, {ci}) tap (dy,dx)=({dy}, {dx}): got {g!r} expected {e!r} [{kind}]; gy pixel (b,h,w)=({b}, {gh}, {gw}) "
                     f"x pixel ({xh}, {xw}): {where}")
    return (f"{int(bad.sum())} of {got.numel()} elements differ from the exact one-hot result; first {len(lines)}:\n" + "\n".join(lines))


def wgrad_ref(x, gy, k: int):
    """(ref, S): dL/dw (cout, cin, k, k) of y = conv2d(x, w) (stride 1, 'same' padding) for dL/dy = gy in float64 on the
    CPU -- torch.nn.grad.conv2d_weight on the operands as the kernel sees them -- and the same sum of absolute values."""
    x64, g64 = x.detach().cpu().double(), gy.detach().cpu().double()
    shape = (g64.shape[1], x64.shape[1], k, k)
    cw = lambda a, g: torch.nn.grad.conv2d_weight(a, shape, g, stride=1, padding=k // 2)
    return cw(x64, g64), cw(x64.abs(), g64.abs())


def assert_wgrad(got, ref, S, what: str, K: int, show: int = 6) -> dict:
    """Every element of the fp32 weight gradient `got` within tau = 2^-20 S of the float64 `ref` (wgrad_ref); a NaN fails
    (dW is NaN-prefilled).  K = B H W, the number of products per element: a case with K 2^-20 > 1/4 is refused, because
    one missing product of ordinary size would then fit inside tau.  Prints the [bounds] summary line; returns its numbers."""
    assert K * TAU_UNIT <= 0.25, (f"{what}: K = {K} products per element: tau = 2^-20 S is {K * TAU_UNIT:.2f} mean products, "
                                  f"more than 1/4 -- the case cannot see one dropped product (K <= {WGRAD_K_CAP})")
    ref, S = ref.detach().cpu().double(), S.detach().cpu().double()
    g, r, s = _np(got), _np(ref), _np(S)
    assert g.shape == r.shape == s.shape, (what, g.shape, r.shape, s.shape)
    tau = TAU_UNIT * s
    ok = np.abs(g - r) <= tau                                     # False for NaN
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(s > 0, np.abs(g - r) / s, np.abs(g - r))
    err = float(np.nanmax(rel)) if rel.size and not np.isnan(rel).all() else float("nan")
    print(f"[bounds] {what}: {g.size} elements, K {K}, max|got-ref|/S {err:.3e} = {err / 2.0 ** -24:.2f} x 2^-24")
    nbad = int((~ok).sum())
    if nbad:
        idx = np.argwhere(~ok)[:show]
        at = lambda a, i: float(a[tuple(i)])
        lines = [f"  (co,ci,dy,dx)={tuple(int(v) for v in i)}: got {at(g, i)!r} ref {at(r, i)!r} tau {at(tau, i):.3e} "
                 f"error {(at(g, i) - at(r, i)) / at(tau, i):+.2f} tau = {(at(g, i) - at(r, i)) * K / at(s, i):+.2f} mean products"
                 for i in idx]
        raise AssertionError(f"{what}: {nbad} of {g.size} elements outside ref -+ 2^-20 S; first {len(idx)}:\n" + "\n".join(lines))
    return {"max_err_over_S": err, "n": int(g.size), "K": K}
