"""Fixed inputs for every kernel of the 16-bit channel-blocked ("C8") path and SHA-256 digests of what codon_amd.ops leaves
for them (tests/test_gpu_c8_bits.py).  The precedent is tests/conv_bits.py: inputs come from the integer hash
of tests/metrics_bits.py alone and only codon_amd._lib / codon_amd.ops names are called, so the module runs unchanged on an
older tree -- which is how tests/golden/c8_bits.json is recorded (python -m tests.c8_bits OUT.json, on the commit BEFORE a
change to the host code that launches these kernels).  The shapes are the smallest that can still go wrong: two images (the
image stride), a width that is no multiple of 32 and a height that is no multiple of 8 or 16 with more than one tile each way
(2 x 19 x 70), every slice at a non-zero channel offset inside a wider buffer.  Only the R = 8 head and the resident conv3x3
need large tensors."""
import ctypes as C
import hashlib
import json
import sys

import torch

from tests.conv_bits import vals, weight

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
SMALL = (2, 19, 70)
STAGED, RESIDENT = 0, 1                 # CODON_C8_FORM_*
CONV_FORMS = [(5, 128, 128), (5, 64, 64), (3, 64, 64), (3, 128, 64), (3, 64, 128), (1, 128, 64), (1, 64, 128)]
GATED_FORMS = [(5, 64, 64), (3, 64, 64), (3, 128, 64)]
# the resident conv3x3 64->64 needs 8 tiles of 32 x 32 per resident workgroup: 256 CUs x 1 workgroup -> 2048 tiles.
# 2 x 32 x 32 tiles is the first launch that has them, one tile row less (2 x 31 x 32 = 1984) the last that has not.
RESIDENT_SHAPE, STAGED_BELOW = (2, 1000, 1000), (2, 992, 1000)
HEAD_R8 = (2, 1450, 1447)               # B H W >= 2^22: bands of 8 rows; below that 4


def _sha(t):
    t = t.detach()
    if t.dtype in (torch.bfloat16, torch.float16):
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()


def act(shape, salt, dtype, scale=1.0):
    """(B, C, H, W) hashed values as an activation buffer of `dtype` (channel-blocked)."""
    from codon_amd import ops
    return ops.from_nchw(vals(shape, salt, scale), dtype)


def big_act(B, C_, H, W, period, salt, dtype):
    """act() for the two large groups: `period` hashed rows repeated down the image (the period divides H and is no multiple of
    a tile height, so no two tiles of a column see the same rows at the same place)."""
    from codon_amd import ops
    assert H % period == 0
    return ops.from_nchw(vals((B, C_, period, W), salt).repeat(1, 1, H // period, 1), dtype)


def form(dtype, B, H, W, k, cin, cout):
    from codon_amd import _lib as L
    dt = {torch.bfloat16: L.BF16, torch.float16: L.F16}[dtype]
    d = L.ConvDesc(B, H, W, cin, cout, k, cin, 0, cout, 0, 0, 0, 0, dt)
    return L.load().codon_conv_form_c8(C.byref(d))


def assert_staged(dtype, B, H, W):
    for k, ci, co in CONV_FORMS:
        assert form(dtype, B, H, W, k, ci, co) == STAGED, (B, H, W, k, ci, co)


# ---- convs ----
def conv_digests(dn):
    """The seven plain shapes under every flag combination codon_conv2d_fwd accepts for 16-bit tensors: the residual slot
    {unused, ADD_RESIDUAL, MASK_RELU} x RELU x ACCUM_OUT = 12, and MASK_RELU | ACCUM_OUT | MASK_SUM (which excludes RELU)."""
    from codon_amd import ops
    from codon_amd.ops import Slice
    dtype, (B, H, W), d = DTYPES[dn], SMALL, {}
    assert_staged(dtype, B, H, W)
    xa, xb, y0 = act((B, 136, H, W), 1, dtype), act((B, 136, H, W), 2, dtype), act((B, 136, H, W), 3, dtype)
    for k, ci, co in CONV_FORMS:
        wp = ops.packed_weight(weight(co, ci, k, 10 + k), dtype=dtype)
        x, r, key = Slice(xa, 8, ci), Slice(xb, 8, co), f"conv_k{k}_{ci}_{co}"
        for name, kw in (("plain", {}), ("relu", dict(relu=True)), ("residual", dict(residual=r)),
                         ("relu_residual", dict(relu=True, residual=r)), ("accum", dict(accumulate=True)),
                         ("relu_accum", dict(relu=True, accumulate=True)), ("residual_accum", dict(residual=r, accumulate=True)),
                         ("mask", dict(relu_mask=r)), ("mask_accum", dict(relu_mask=r, accumulate=True)),
                         ("mask_accum_sum", dict(relu_mask=r, accumulate=True, mask_sum=True)),
                         ("relu_residual_accum", dict(relu=True, residual=r, accumulate=True)),
                         ("relu_mask", dict(relu=True, relu_mask=r)),
                         ("relu_mask_accum", dict(relu=True, relu_mask=r, accumulate=True))):
            y = y0.clone()
            ops.conv2d(x, wp, Slice(y, 8, co), k, **kw)
            d[f"{key}_{name}"] = _sha(y)                          # the whole buffer: the planes beside the slice stay
    return d


def gated_digests(dn):
    from codon_amd import ops
    from codon_amd.ops import Slice
    dtype, (B, H, W), d = DTYPES[dn], SMALL, {}
    xa, xb = act((B, 192, H, W), 4, dtype), act((B, 192, H, W), 5, dtype)
    ch, sp = vals((B, 64), 6) + 0.5, vals((B, 1, H, W), 7) + 0.5
    for k, ci, co in GATED_FORMS:
        wp = ops.packed_weight(weight(co, ci, k, 20 + k), dtype=dtype)
        key = f"gated_k{k}_{ci}_{co}"
        for relu in (False, True):
            y = act((B, co + 8, H, W), 8, dtype)
            ops.conv2d_gated(Slice(xa, 64, ci), Slice(xb, 8, ci), ch, sp, wp, Slice(y, 8, co), k, relu=relu)
            d[f"{key}_relu{int(relu)}"] = _sha(y)
        y, em = act((B, co + 8, H, W), 8, dtype), act((B, ci + 8, H, W), 9, dtype)
        ops.conv2d_gated(Slice(xa, 64, ci), Slice(xb, 8, ci), ch, sp, wp, Slice(y, 8, co), k, relu=True, emit=Slice(em, 8, ci))
        d[key + "_emit_y"], d[key + "_emit_x"] = _sha(y), _sha(em)
    return d


def chain_digests(dn):
    from codon_amd import _lib as L, ops
    from codon_amd.ops import Slice
    dtype, (B, H, W), d = DTYPES[dn], SMALL, {}
    xa, xb = act((B, 136, H, W), 11, dtype), act((B, 136, H, W), 12, dtype)
    w5 = ops.packed_weight(weight(128, 128, 5, 30), dtype=dtype)
    w1 = ops.packed_weight(weight(64, 128, 1, 31), L.PACK_CHAIN1X1, dtype=dtype)
    nparts = ops.cac_fused_parts(H, W, dtype)
    assert nparts == ops.cac_fused_tiles(H, W) == 3 * 3
    for mid in (0, 1):
        for res in (0, 1):
            for st in (None, 0, 64):
                out, m = act((B, 72, H, W), 13, dtype), act((B, 136, H, W), 14, dtype)
                pool, part = vals((B, 2, H, W), 15), vals((B, nparts, 128, 2), 16)
                ops.conv_chain1x1(Slice(xa, 8, 128), w5, w1, Slice(out, 8, 64), mid=Slice(m, 8, 128) if mid else None,
                                  residual=Slice(xb, 16, 64) if res else None, stats=None if st is None else (pool, part, st))
                key = f"chain_mid{mid}_res{res}_stats{st}"
                d[key + "_out"] = _sha(out)
                if mid:
                    d[key + "_mid"] = _sha(m)
                if st is not None:
                    d[key + "_pool"], d[key + "_partials"] = _sha(pool), _sha(part)
    return d


def sum_into_digests(dn):
    """Outside a pair bracket, and inside an open one: the call launches at once either way (it is never held back), so the
    bracket closes with no launch of its own."""
    from codon_amd import ops
    from codon_amd.ops import Slice
    dtype, (B, H, W), d = DTYPES[dn], SMALL, {}
    xa = act((B, 72, H, W), 17, dtype)
    wp = ops.packed_weight(weight(64, 64, 5, 32), dtype=dtype)
    for acc in (False, True):
        for inside in (False, True):
            y, tot = act((B, 72, H, W), 18, dtype), act((B, 72, H, W), 19, dtype)
            with ops.conv_pair(xa.device, enabled=inside) as br:
                ops.conv2d_sum_into(Slice(xa, 8, 64), wp, Slice(y, 8, 64), 5, Slice(tot, 8, 64), accumulate=acc)
            key = f"sum_into_acc{int(acc)}_pair{int(inside)}"
            d[key + "_y"], d[key + "_total"] = _sha(y), _sha(tot)
            if inside:
                d[key + "_launches"] = br.launches
    return d


def pair_digests(dn):
    """Two calls of one kernel in a bracket (one launch), the 5x5 + 3x3 siblings (one mix53 launch), two chained convs."""
    from codon_amd import _lib as L, ops
    from codon_amd.ops import Slice
    dtype, (B, H, W), d = DTYPES[dn], SMALL, {}
    xa, xb = act((B, 136, H, W), 21, dtype), act((B, 136, H, W), 22, dtype)
    dev = xa.device
    w5, w3 = ops.packed_weight(weight(64, 64, 5, 33), dtype=dtype), ops.packed_weight(weight(64, 64, 3, 34), dtype=dtype)
    for k, wp in ((5, w5), (3, w3)):
        o = act((B, 136, H, W), 23, dtype)
        with ops.conv_pair(dev) as br:
            ops.conv2d(Slice(xa, 8, 64), wp, Slice(o, 8, 64), k, relu=True)
            ops.conv2d(Slice(xa, 72, 64), wp, Slice(o, 72, 64), k, relu=True)
        d[f"pair_k{k}"], d[f"pair_k{k}_launches"] = _sha(o), br.launches
    for order in ("53", "35"):
        o = act((B, 136, H, W), 24, dtype)
        with ops.conv_pair(dev) as br:
            for k in order:
                ops.conv2d(Slice(xb, 72, 64), w5 if k == "5" else w3, Slice(o, 8 if k == "5" else 72, 64), int(k), relu=True)
        d[f"mix{order}"], d[f"mix{order}_launches"] = _sha(o), br.launches
    wc5 = ops.packed_weight(weight(128, 128, 5, 35), dtype=dtype)
    wc1 = ops.packed_weight(weight(64, 128, 1, 36), L.PACK_CHAIN1X1, dtype=dtype)
    o = act((B, 136, H, W), 25, dtype)
    with ops.conv_pair(dev) as br:
        ops.conv_chain1x1(Slice(xa, 8, 128), wc5, wc1, Slice(o, 8, 64))
        ops.conv_chain1x1(Slice(xb, 8, 128), wc5, wc1, Slice(o, 72, 64), residual=Slice(xa, 16, 64))
    d["pair_chain"], d["pair_chain_launches"] = _sha(o), br.launches
    return d


def resident_digests(dn):
    from codon_amd import ops
    from codon_amd.ops import Slice
    dtype, (B, H, W) = DTYPES[dn], RESIDENT_SHAPE
    assert form(dtype, B, H, W, 3, 64, 64) == RESIDENT
    assert form(dtype, *STAGED_BELOW, 3, 64, 64) == STAGED
    for k, ci, co in CONV_FORMS:
        assert (k, ci, co) == (3, 64, 64) or form(dtype, B, H, W, k, ci, co) == STAGED
    x, y = big_act(B, 72, H, W, 125, 26, dtype), ops.new_act(B, 72, H, W, dtype, "cuda").zero_()
    wp = ops.packed_weight(weight(64, 64, 3, 37), dtype=dtype)
    ops.conv2d(Slice(x, 8, 64), wp, Slice(y, 8, 64), 3, relu=True)
    return {"resident_k3_64_64_relu": _sha(y)}


# ---- stems and heads ----
def stem_digests(dn):
    from codon_amd import ops
    from codon_amd.ops import Slice
    dtype, (B, H, W), d = DTYPES[dn], (2, 19, 150), {}        # two 128-column segments, the second ragged
    xa, xb = vals((B, 1, H, W), 41), vals((B, 1, H, W), 42)
    wa, wb = vals((64, 1, 3, 3), 43), vals((64, 1, 3, 3), 44)
    y = act((B, 136, H, W), 45, dtype)
    ops.stem(xa, wa, Slice(y, 8, 64))
    d["stem"] = _sha(y)
    mask = act((B, 72, H, W), 46, dtype)
    for relu in (False, True):
        for flip in (False, True):
            for m in (None, Slice(mask, 8, 64)):
                y = act((B, 136, H, W), 45, dtype)
                ops.stencil_1to64(xa, wa.reshape(64, 9), Slice(y, 72, 64), relu=relu, flip=flip, mask=m)
                d[f"stencil_relu{int(relu)}_flip{int(flip)}_mask{int(m is not None)}"] = _sha(y)
    y = act((B, 136, H, W), 45, dtype)
    ops.stem_pair(xa, wa, Slice(y, 72, 64), xb, wb, Slice(y, 8, 64))
    d["stem_pair"] = _sha(y)
    return d


def _head(dn, B, H, W):
    from codon_amd import ops
    from codon_amd.ops import Slice
    dtype = DTYPES[dn]
    x, w, res = big_act(B, 72, H, W, 50 if H % 50 == 0 else H, 47, dtype), vals((1, 64, 3, 3), 48), vals((B, 1, H, W), 49)
    y = torch.zeros((B, 1, H, W), device="cuda")
    ops.head(Slice(x, 8, 64), w, res, y)
    y16 = torch.zeros((B, 1, H, W), device="cuda", dtype=dtype)
    ops.head(Slice(x, 8, 64), w, res, y16)
    return {"head": _sha(y), "head_y16": _sha(y16)}


def head_digests(dn):
    return _head(dn, 2, 19, 70)                               # two 62-column segments, bands of 4 rows, the last ragged


def head_r8_digests(dn):
    B, H, W = HEAD_R8
    assert B * H * W >= 1 << 22 and H % 8 and W % 62 and H % 50 == 0
    return _head(dn, B, H, W)


def conv1ch_wgrad_digests(dn):
    from codon_amd import ops
    from codon_amd.ops import Slice
    dtype, (B, H, W), d = DTYPES[dn], SMALL, {}
    a, s = act((B, 72, H, W), 51, dtype), vals((B, 1, H, W), 52)
    for flip in (False, True):
        dw = torch.zeros(576, device="cuda"); ops.conv1ch_wgrad(Slice(a, 8, 64), s, dw, flip); d[f"flip{int(flip)}_immediate"] = _sha(dw)
        dw = vals((576,), 53); ops.conv1ch_wgrad(Slice(a, 8, 64), s, dw, flip, accumulate=True); d[f"flip{int(flip)}_accumulate"] = _sha(dw)
        dw, dr = torch.zeros(576, device="cuda"), ops.DeferredReduce()
        ops.conv1ch_wgrad(Slice(a, 8, 64), s, None, flip, defer=(dr, "w")); dr.run({"w": dw}, accumulate=False)
        d[f"flip{int(flip)}_deferred"] = _sha(dw)
    return d


# ---- CAC gate and elementwise kernels ----
def cac_fwd_digests(dn):
    from codon_amd import ops
    from codon_amd.ops import Slice
    dtype, d = DTYPES[dn], {}
    for B, H, W in (SMALL, (2, 130, 257)):                    # 256-pixel tiles up to 32768 pixels, 2048-pixel ones above
        tag = f"{B}x{H}x{W}"
        nt = ops.cac_stats_tiles(H, W)
        assert nt == (-(-H * W // 256) if H * W <= 32768 else -(-H * W // 2048)) and nt > 1
        pc, pd = act((B, 72, H, W), 61, dtype), act((B, 136, H, W), 62, dtype)
        ch = vals((B, 64), 63) + 0.5
        pooled, part = vals((B, 2, H, W), 64), vals((B, nt, 128, 2), 65)
        ops.cac_stats(Slice(pc, 8, 64), Slice(pd, 72, 64), pooled, part)
        d[f"stats_{tag}_pooled"], d[f"stats_{tag}_partials"] = _sha(pooled), _sha(part)
        pooled, part = vals((B, 2, H, W), 64), vals((B, nt, 128, 2), 65)
        ops.cac_stats_scaled(Slice(pc, 8, 64), Slice(pd, 72, 64), ch, pooled, part)
        d[f"stats_scaled_{tag}_pooled"] = _sha(pooled)            # only `pooled` is meaningful (include/codon_hip.h)
    B, H, W = 2, 19, 70 + 1024 // 19                              # more than one 1024-pixel tile of cac_apply
    pre, inp, out = act((B, 136, H, W), 66, dtype), act((B, 136, H, W), 67, dtype), act((B, 144, H, W), 68, dtype)
    ch, sp = vals((B, 64), 63) + 0.5, vals((B, 1, H, W), 69) + 0.5
    ops.cac_apply(Slice(pre, 72, 64), Slice(pre, 8, 64), ch, sp, Slice(inp, 72, 64), Slice(inp, 8, 64), Slice(out, 80, 64),
                  Slice(out, 8, 64))
    d["apply"] = _sha(out)
    y = act((B, 72, H, W), 70, dtype)
    ops.ew_sq_scale(Slice(pre, 8, 64), ch, Slice(y, 8, 64))
    d["sq_scale"] = _sha(y)
    return d


def ew_digests(dn):
    from codon_amd import ops
    from codon_amd.ops import Slice
    dtype, (B, H, W), d = DTYPES[dn], SMALL, {}
    src = [act((B, 136, H, W), 71 + i, dtype) for i in range(4)]
    mask = act((B, 136, H, W), 75, dtype)
    for C_ in (64, 128):
        for has_src in (0, 1):
            for has_mask in (0, 1):
                for acc in (0, 1):
                    if not has_src and not has_mask:
                        continue
                    dst = act((B, 136, H, W), 76, dtype)
                    ops.ew_add_mask(Slice(dst, 8, C_), Slice(src[0], 8, C_) if has_src else None,
                                    Slice(mask, 8, C_) if has_mask else None, accumulate=bool(acc))
                    d[f"add_mask_c{C_}_src{has_src}_mask{has_mask}_acc{acc}"] = _sha(dst)
        for n in (1, 2, 3, 4):
            for has_mask in (0, 1):
                dst = act((B, 136, H, W), 76, dtype)
                ops.ew_sum_mask(Slice(dst, 8, C_), [Slice(s, 8, C_) for s in src[:n]], Slice(mask, 8, C_) if has_mask else None)
                d[f"sum_mask_c{C_}_n{n}_mask{has_mask}"] = _sha(dst)
    return d


def cac_bwd_digests(dn):
    """ops.cac_backward = cac_bwd_reduce + gate + spatial + cac_bwd_apply (both accumulate_in forms); ops.cac_backward_fused =
    cac_bwd_reduce_acc (accumulate_in 0, 1, 2) + gate + spatial."""
    from codon_amd import ops
    from codon_amd.ops import Slice
    dtype, (B, H, W), d = DTYPES[dn], (2, 19, 130), {}          # two 2048-pixel tiles
    g, p = act((B, 136, H, W), 81, dtype), act((B, 136, H, W), 82, dtype)
    ch, sp = vals((B, 64), 83) + 0.5, vals((B, 1, H, W), 84) + 0.5
    pooled, pools = vals((B, 2, H, W), 85), vals((B, 2, 128), 86)
    w1, b1, w2, ws = vals((8, 128), 87), vals((8,), 88), vals((64, 8), 89), vals((1, 2, 5, 5), 90)
    names = ("dw1", "db1", "dw2", "db2", "dws")
    args = (Slice(g, 72, 64), Slice(g, 8, 64), Slice(p, 72, 64), Slice(p, 8, 64), ch, sp, pooled, pools, w1, b1, w2, ws)
    for acc in (0, 1):
        gp, gi = act((B, 136, H, W), 91, dtype), act((B, 136, H, W), 92, dtype)
        outs = ops.cac_backward(*args, Slice(gp, 72, 64), Slice(gp, 8, 64), Slice(gi, 72, 64), Slice(gi, 8, 64), bool(acc))
        d[f"bwd_acc{acc}_g_pre"], d[f"bwd_acc{acc}_g_in"] = _sha(gp), _sha(gi)
        for n, t in zip(names, outs):
            d[f"bwd_acc{acc}_{n}"] = _sha(t)
    for acc in (0, 1, 2):
        gi = act((B, 136, H, W), 92, dtype)
        outs = ops.cac_backward_fused(*args, Slice(gi, 72, 64), Slice(gi, 8, 64), acc)
        d[f"fused_acc{acc}_g_in"] = _sha(gi)
        for n, t in zip(names, outs[:5]):
            d[f"fused_acc{acc}_{n}"] = _sha(t)
        for n in ("g_pooled", "g_pools", "argpix", "argch"):
            d[f"fused_acc{acc}_{n}"] = _sha(outs[5][n])
    return d


KINDS = {"conv": conv_digests, "gated": gated_digests, "chain": chain_digests, "sum_into": sum_into_digests,
         "pair": pair_digests, "resident": resident_digests, "stem": stem_digests, "head": head_digests,
         "head_r8": head_r8_digests, "conv1ch_wgrad": conv1ch_wgrad_digests, "cac_fwd": cac_fwd_digests, "ew": ew_digests,
         "cac_bwd": cac_bwd_digests}
GROUPS = [(k, dn) for k in KINDS for dn in DTYPES]
EXCLUDED = []                           # groups whose kernels use floating-point atomics: none does


def group_digests(kind, dn):
    return KINDS[kind](dn)


def group_id(kind, dn):
    return f"{kind}_{dn}"


def digests():
    """{group id: {case: sha256 of the raw little-endian bytes of the output, or a launch count}}."""
    return {group_id(k, dn): group_digests(k, dn) for k, dn in GROUPS}


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(digests(), f, indent=1, sort_keys=True)
        f.write("\n")
