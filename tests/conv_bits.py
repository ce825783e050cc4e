"""Fixed inputs for the fp32 forward convs and the weight-gradient kernels, and SHA-256 digests of what codon_amd.ops leaves
for them (tests/test_gpu_conv_bits.py), plus the table of codon_conv_tiling_f32 over a grid of shapes
(tests/test_conv_tiling_table.py).  The precedent is tests/metrics_bits.py: inputs come from its integer hash alone, only
ops names are called, so the module runs unchanged on an older tree -- which is how tests/golden/conv_bits.json and
tests/golden/f32_tiling.json are recorded (python -m tests.conv_bits bits OUT.json / tiling OUT.json, on the commit BEFORE a
change to the host code that launches these kernels).  Every group of cases first asserts, through codon_conv_tiling_f32 or
tests.bounds.wgrad_bands, the tiling or band plan its shape is there for.  Also here: the batches of one small image that
select each fp32 tiling, the exact power-of-two batch construction and the bit comparison of tests/test_gpu_f32_tilings.py."""
import ctypes as C
import hashlib
import json
import sys

import numpy as np
import torch

from tests.metrics_bits import hash16

T8, T4, SOLO, SPLIT = 0, 1, 2, 3       # CODON_TILING_8X32, _4X32, _4X32_SOLO, _2X32_COUT_SPLIT

# ---- the tiling table (host arithmetic, no GPU) ----
TILING_BATCH = [1, 2, 3, 5, 8, 32]
TILING_HW = [(8, 8), (64, 64), (128, 128), (128, 160), (128, 200), (247, 343), (300, 463), (370, 463), (440, 463), (480, 463),
             (480, 640), (820, 463), (960, 1280), (1920, 2560)]
TILING_FORMS = [(5, 128, 128, 1), (5, 128, 128, 0), (5, 64, 64, 0), (3, 64, 64, 0), (3, 128, 64, 0), (3, 64, 128, 0),
                (1, 128, 64, 0), (1, 64, 128, 0)]          # (k, cin, cout, chained)


def tiling(B, H, W, k, cin, cout, chained, in_pair):
    from codon_amd import _lib as L
    d = L.ConvDesc(B, H, W, cin, cout, k, cin, 0, cout, 0, 0, 0, 0, L.F32)
    return L.load().codon_conv_tiling_f32(C.byref(d), chained, in_pair)


def tiling_table():
    """{"k<k>_<cin>_<cout>_chained<c>_pair<p>": one digit per (batch, (H, W)), batch outermost}."""
    return {f"k{k}_{ci}_{co}_chained{ch}_pair{p}":
            "".join(str(tiling(B, H, W, k, ci, co, ch, p)) for B in TILING_BATCH for H, W in TILING_HW)
            for k, ci, co, ch in TILING_FORMS for p in (0, 1)}


# ---- one small image, the batch selects the tiling (tests/test_gpu_f32_tilings.py; premises: tests/test_conv_tiling_table.py) ----
TILING_NAME = {T8: "T8", T4: "T4", SOLO: "SOLO", SPLIT: "SPLIT"}
TILE_ROWS = {T8: 8, T4: 4, SOLO: 4, SPLIT: 2}          # f32_fill: pixel rows of a tile; every tile is 32 pixels wide
TILE_COLS = 32
# A: ragged -- 3 tile columns, the last 6 pixels wide; last tile rows of 5 of 8, 1 of 4 and 1 of 2 rows; no block count below is
# a multiple of 8.  B: exact tiles, W % 4 == 0, every row starts on 16 bytes.
GEOMETRY = {"A": (13, 70), "B": (16, 64)}
# (geometry, batch) -> what the case is there for: the tiling of (the chained conv, a plain 5x5, a plain 3x3, a 1x1) outside a
# pair bracket, and inside one.  What the library answers is asked, never computed here: tiling_premise.
BATCH_TILING = {("A", 1): ((SPLIT, SPLIT, SPLIT, SOLO),) * 2,
                ("A", 5): ((SPLIT, SPLIT, SPLIT, SOLO),) * 2,          # a cout-split pair of 210 workgroups: <= 256, padded
                ("A", 8): ((SPLIT, SPLIT, SPLIT, SOLO),) * 2,          # ... of 336: two to a CU, no padding
                ("A", 12): ((SPLIT, SPLIT, SPLIT, SOLO), (SOLO,) * 4),  # 144 tiles of 4 x 32: <= 192 alone, > 128 in a pair
                ("A", 17): ((SOLO,) * 4,) * 2,                         # 204 > 192
                ("A", 65): ((T8,) * 4,) * 2,                           # 390 tiles of 8 x 32 >= 384, one round
                ("A", 107): ((T4, T4, T8, T8),) * 2,                   # 642 tiles of 8 x 32: two rounds, three of 4 x 32
                ("B", 1): ((SPLIT, SPLIT, SPLIT, SOLO),) * 2,
                ("B", 25): ((SOLO,) * 4,) * 2,                         # 200 > 192
                ("B", 97): ((T8,) * 4,) * 2,                           # 388 >= 384
                ("B", 161): ((T4, T4, T8, T8),) * 2}                   # 644
PAIR_GRID_LIMIT = 256                                  # launch_pair_f32: a cout-split pair of at most this many workgroups is padded


def tiling_premise(geo, B, k, cin, cout, chained=0, in_pair=0):
    """The tiling codon_conv_tiling_f32 gives the launch (cin -> cout as its descriptor has them), asserted to be the one the
    case (geo, B) is there for."""
    H, W = GEOMETRY[geo]
    want = BATCH_TILING[geo, B][in_pair][0 if chained else {5: 1, 3: 2, 1: 3}[k]]
    got = tiling(B, H, W, k, cin, cout, chained, in_pair)
    assert got == want, (f"premise: {B}x{H}x{W} k={k} {cin}->{cout} chained={chained} in_pair={in_pair} runs "
                         f"{TILING_NAME[got]}, the case is there for {TILING_NAME[want]}")
    return got


def assert_batch_tiling(geo, B):
    for p in (0, 1):
        for k, ci, co, ch in TILING_FORMS:
            tiling_premise(geo, B, k, ci, co, ch, p)


def batch_exponents(B):
    """(base image, exponent) of every image of a batch of B: image b is base[b % 3] * 2^(b // 3 - E), E half the largest b // 3."""
    b = np.arange(B)
    return b % 3, b // 3 - ((B - 1) // 3) // 2


def expand(base, B, imgs=None, scaled=True):
    """base (3, ...) -> the images `imgs` (default: all) of the batch of B built from it; on base's device, in its dtype.
    A power-of-two scale: exact unless something under- or overflows (|exponent| <= 27 here)."""
    idx, e = batch_exponents(B)
    if imgs is not None:
        idx, e = idx[list(imgs)], e[list(imgs)]
    out = base[torch.from_numpy(idx).to(base.device)]
    if scaled:
        s = torch.from_numpy(2.0 ** e.astype(np.float64)).to(device=base.device, dtype=base.dtype)
        out = out * s.reshape((-1,) + (1,) * (base.dim() - 1))
    return out


def probe_images(B):
    """The first, a middle and the last image of a batch, the middle one on another base image where there is one."""
    if B < 3:
        return list(range(B))
    mid = B // 2
    while mid % 3 in (0, (B - 1) % 3) and mid + 1 < B - 1:
        mid += 1
    return [0, mid, B - 1]


def tile_where(t, H, W, h, w):
    """'T8: band j of n (rows a..b), segment s of m (columns c..d)' of pixel (h, w) under tiling t (tests.forms.where), and
    the wave and row segment that own the row."""
    from tests import forms
    th = TILE_ROWS[t]
    form = {"bands": forms._spans(H, th), "segs": forms._spans(W, TILE_COLS)}
    own = (f"wave {h % th // 2}, row segment {h % 2} of 2" if t == T8 else
           f"waves {h % th} and {h % th + 2} (halves of the couts)" if t == SPLIT else f"wave {h % th}")
    return f"{TILING_NAME[t]}: {forms.where(form, h, w)}, {own}"


def bits_mismatch(got, base, B, t, H, W, what, show=6, col_step=1):
    """None when image b of `got` (B, C, h, w) equals base[b % 3] * 2^(b // 3 - E) bit for bit -- base (3, C, h, w): the results
    for the three base images run alone -- else a message naming the first differing elements: image, channel, pixel, its
    tile under tiling t, both values.  Compared on got's device.  col_step: pixels per element along the last axis (32 for
    the row-strip statistics, whose last axis counts tile columns)."""
    exp = expand(base, B)
    assert got.shape == exp.shape, (what, tuple(got.shape), tuple(exp.shape))
    if torch.equal(got, exp):
        return None
    bad = ~(got == exp)                                                # a NaN on either side differs
    idx = bad.nonzero()[:show].cpu().tolist()
    _, e = batch_exponents(B)
    lines = [f"  image {b} (base image {b % 3} x 2^{int(e[b])}) channel {c} pixel ({h}, {w * col_step}): got {float(got[b, c, h, w])!r} "
             f"expected {float(exp[b, c, h, w])!r}; {tile_where(t, H, W, h, w * col_step)}" for b, c, h, w in idx]
    return (f"{what}: {int(bad.sum())} of {got.numel()} elements differ from the single-image result scaled by a power of two; "
            f"first {len(lines)}:\n" + "\n".join(lines))


# ---- inputs ----
def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def vals(shape, salt, scale=1.0):
    """float32 cuda tensor of hashed values in [-scale / 2, scale / 2) on a grid of 2^-16 * scale (exact in bf16 only by luck)."""
    n = int(np.prod(shape))
    v = (hash16(n, salt).astype(np.float32) - np.float32(32768)) * np.float32(scale / 65536)
    return torch.from_numpy(v.reshape(shape)).cuda()


def weight(cout, cin, k, salt):
    return vals((cout, cin, k, k), salt, 2.0 * (2.0 / (k * k * cin)) ** 0.5)


# ---- fp32 forward ----
FWD_SHAPES = [(1, 6, 40), (1, 128, 160), (1, 128, 200), (1, 370, 463), (1, 480, 463)]
PAIR_SHAPES = FWD_SHAPES[:2]
CONV_FORMS = [(5, 128, 128), (5, 64, 64), (3, 64, 64), (3, 128, 64), (3, 64, 128), (1, 128, 64), (1, 64, 128)]
GATED_FORMS = [(5, 64, 64), (3, 64, 64), (3, 128, 64)]
# (H, W) -> tiling of (the chained conv, a plain 5x5, a plain 3x3, a 1x1) outside a pair bracket, and inside one
FWD_TILING = {(6, 40): ((SPLIT, SPLIT, SPLIT, SOLO), (SPLIT, SPLIT, SPLIT, SOLO)),     # 4 tiles of 4 x 32, ragged both ways
              (128, 160): ((SPLIT, SPLIT, SPLIT, SOLO), (SOLO, SOLO, SOLO, SOLO)),     # 160 tiles: <= 192 alone, > 128 per pair launch
              (128, 200): ((SOLO,) * 4, (SOLO,) * 4),                                  # 224 tiles of 4 x 32 > 192
              (370, 463): ((T4, T4, T8, T8), (T4, T4, T8, T8)),                        # 705 tiles of 8 x 32: two per CU in 4 x 32
              (480, 463): ((T8,) * 4, (T8,) * 4)}                                      # 900 tiles


def assert_fwd_tiling(B, H, W):
    for p in (0, 1):
        chain, k5, k3, k1 = FWD_TILING[(H, W)][p]
        assert tiling(B, H, W, 5, 128, 128, 1, p) == chain, (H, W, p)
        for k, ci, co in CONV_FORMS:                      # the gated convs take the plain rule of their shape
            assert tiling(B, H, W, k, ci, co, 0, p) == {5: k5, 3: k3, 1: k1}[k], (H, W, k, ci, co, p)


def forward_digests(B, H, W):
    from codon_amd import _lib as L, ops
    from codon_amd.ops import Slice
    assert_fwd_tiling(B, H, W)
    d, tag = {}, f"{B}x{H}x{W}"
    xa, xb = vals((B, 128, H, W), 1), vals((B, 128, H, W), 2)
    new = lambda c: torch.zeros((B, c, H, W), device="cuda")
    for k, ci, co in CONV_FORMS:
        wp = ops.packed_weight(weight(co, ci, k, 10 + k))
        x, key = Slice(xa, 128 - ci, ci), f"conv_k{k}_{ci}_{co}_{tag}"
        y = new(co); ops.conv2d(x, wp, Slice(y), k); d[key + "_plain"] = _sha(y)
        y = new(co); ops.conv2d(x, wp, Slice(y), k, relu=True); d[key + "_relu"] = _sha(y)
        y = new(co); ops.conv2d(x, wp, Slice(y), k, residual=Slice(xb, 0, co)); d[key + "_residual"] = _sha(y)
        y = xb[:, 128 - co:].clone()
        ops.conv2d(x, wp, Slice(y), k, relu_mask=Slice(xa, 0, co), accumulate=True, mask_sum=True)
        d[key + "_masksum"] = _sha(y)
    ch, sp = vals((B, 64), 3) + 0.5, vals((B, 1, H, W), 4) + 0.5
    for k, ci, co in GATED_FORMS:
        wp = ops.packed_weight(weight(co, ci, k, 20 + k))
        key = f"gated_k{k}_{ci}_{co}_{tag}"
        y = new(co)
        ops.conv2d_gated(Slice(xa, 128 - ci, ci), Slice(xb, 128 - ci, ci), ch, sp, wp, Slice(y), k, relu=True)
        d[key] = _sha(y)
        y, em = new(co), new(ci + 8)
        ops.conv2d_gated(Slice(xa, 128 - ci, ci), Slice(xb, 128 - ci, ci), ch, sp, wp, Slice(y), k, emit=Slice(em, 8, ci))
        d[key + "_emit_y"], d[key + "_emit_x"] = _sha(y), _sha(em)
    w5, w1 = ops.packed_weight(weight(128, 128, 5, 30)), ops.packed_weight(weight(64, 128, 1, 31), L.PACK_CHAIN1X1)
    nparts = ops.cac_fused_parts(H, W, torch.float32)
    for name, mid, res, st in (("plain", 0, 0, 0), ("mid", 1, 0, 0), ("residual", 0, 1, 0), ("mid_residual", 1, 1, 0),
                               ("stats", 0, 0, 1), ("mid_stats", 1, 0, 1)):
        out, m = new(64), new(128) if mid else None
        pool, part = new(2), torch.zeros((B, nparts, 128, 2), device="cuda")
        ops.conv_chain1x1(Slice(xa), w5, w1, Slice(out), mid=Slice(m) if mid else None,
                          residual=Slice(xb, 64, 64) if res else None, stats=(pool, part, 64) if st else None)
        key = f"chain_{name}_{tag}"
        d[key + "_out"] = _sha(out)
        if mid:
            d[key + "_mid"] = _sha(m)
        if st:
            d[key + "_pool"], d[key + "_partials"] = _sha(pool), _sha(part)
    return d


def pair_digests(B, H, W):
    """Inside ops.conv_pair: two calls of one kernel (the chained conv, the 5x5 and the 3x3 64 -> 64) and the 5x5 + 3x3 siblings
    on one input; both outputs and the number of launches the bracket took."""
    from codon_amd import _lib as L, ops
    from codon_amd.ops import Slice
    assert_fwd_tiling(B, H, W)
    d, tag = {}, f"{B}x{H}x{W}"
    xa, xb = vals((B, 128, H, W), 5), vals((B, 128, H, W), 6)
    dev = xa.device
    new = lambda c: torch.zeros((B, c, H, W), device="cuda")
    w5, w1 = ops.packed_weight(weight(128, 128, 5, 40)), ops.packed_weight(weight(64, 128, 1, 41), L.PACK_CHAIN1X1)
    w5b = ops.packed_weight(weight(128, 128, 5, 42))
    o = new(128)
    with ops.conv_pair(dev) as br:
        ops.conv_chain1x1(Slice(xa), w5, w1, Slice(o, 0, 64))
        ops.conv_chain1x1(Slice(xb), w5b, w1, Slice(o, 64, 64), residual=Slice(xa, 64, 64))
    d[f"pair_chain_{tag}"], d[f"pair_chain_{tag}_launches"] = _sha(o), br.launches
    w564, w364 = ops.packed_weight(weight(64, 64, 5, 43)), ops.packed_weight(weight(64, 64, 3, 44))
    for k, wp in ((5, w564), (3, w364)):
        o = new(128)
        with ops.conv_pair(dev) as br:
            ops.conv2d(Slice(xa, 0, 64), wp, Slice(o, 0, 64), k, relu=True)
            ops.conv2d(Slice(xa, 64, 64), wp, Slice(o, 64, 64), k, relu=True)
        d[f"pair_k{k}_{tag}"], d[f"pair_k{k}_{tag}_launches"] = _sha(o), br.launches
    o = new(128)
    with ops.conv_pair(dev) as br:                          # conv8 | conv9 of the fusion trunk
        ops.conv2d(Slice(xb, 64, 64), w564, Slice(o, 0, 64), 5, relu=True)
        ops.conv2d(Slice(xb, 64, 64), w364, Slice(o, 64, 64), 3, relu=True)
    d[f"pair_siblings_{tag}"], d[f"pair_siblings_{tag}_launches"] = _sha(o), br.launches
    return d


# ---- weight gradients ----
WGRAD_FORMS = [(5, 128, 128), (5, 64, 64), (3, 64, 64), (3, 128, 64), (1, 128, 64)]
WGRAD_F32 = [((2, 36, 40), "f32_t16"), ((2, 37, 41), "f32_r1")]
WGRAD_16 = [(1, 130, 40), (3, 37, 53)]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def assert_wgrad_plan(dtype, k, cin, cout, B, H, W, kernel):
    """The plan tests.bounds.wgrad_bands restates is the one the library sizes its workspace for, runs `kernel`, and is the
    case the shape is there for: several bands; the round-1 kernel with a clipped last tile row; thirteen one-tile bands."""
    from codon_amd import _lib as L
    from tests import bounds
    plan = bounds.wgrad_bands(dtype, k, cin, cout, B, H, W)
    dt = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}[dtype]
    d = L.ConvDesc(B, H, W, cin, cout, k, cin, 0, cout, 0, 0, 0, 0, dt)
    assert L.load().codon_conv_wgrad_workspace_bytes(C.byref(d)) == plan["nsplit"] * cout * cin * k * k * 4, plan
    assert plan["kernel"] == kernel and plan["nbands"] > 1, plan
    if kernel == "f32_r1":
        assert plan["bands"][-1][1] * plan["th"] > H, plan                 # ragged last band
    if kernel == "c8" and k == 5 and (B, H, W) == (1, 130, 40):
        assert plan["rows_per_band"] == [1] * 13, plan
    return plan


def _three_forms(run, dw_shape, salt):
    """run(dw, accumulate, defer) in immediate, accumulate and deferred form -> the three dw digests."""
    from codon_amd import ops
    out = []
    dw = torch.zeros(dw_shape, device="cuda"); run(dw, False, None); out.append(_sha(dw))
    dw = vals(dw_shape, salt); run(dw, True, None); out.append(_sha(dw))
    dw, dr = torch.zeros(dw_shape, device="cuda"), ops.DeferredReduce()
    run(None, False, (dr, "w")); dr.run({"w": dw}, accumulate=False); out.append(_sha(dw))
    return dict(zip(("immediate", "accumulate", "deferred"), out))


def wgrad_digests(dname, B, H, W, kernel):
    from codon_amd import _lib as L, ops
    from codon_amd.ops import Slice
    dtype, d, tag = DTYPES[dname], {}, f"{dname}_{B}x{H}x{W}"
    x2 = ops.from_nchw(vals((B, 128, H, W), 50).clamp_min(0), dtype)        # a ReLU output (conv1x1_bwd masks by it)
    g2 = ops.from_nchw(vals((B, 128, H, W), 51), dtype)
    for k, ci, co in WGRAD_FORMS:
        assert_wgrad_plan(dtype, k, ci, co, B, H, W, kernel)
        run = lambda dw, acc, defer: ops.conv2d_wgrad(Slice(x2, 128 - ci, ci), Slice(g2, 128 - co, co), dw, k,
                                                      accumulate=acc, defer=defer)
        for form, h in _three_forms(run, (co, ci, k, k), 52).items():
            d[f"wgrad_k{k}_{ci}_{co}_{tag}_{form}"] = h
    if dname == "f32":
        return d
    wd = ops.packed_weight(weight(64, 128, 1, 53), mode=L.PACK_DGRAD, dtype=dtype)
    gate = dict(ch=vals((B, 64), 54) + 0.5, sp=vals((B, 1, H, W), 55) + 0.5, g_pooled=vals((B, 2, H, W), 56),
                g_pools=vals((B, 2, 128), 57),
                argpix=torch.from_numpy((hash16(B * 128, 58) % (H * W)).astype(np.int32).reshape(B, 128)).cuda(),
                argch=torch.from_numpy((hash16(B * H * W, 59) % 128).astype(np.int32).reshape(B, H, W)).cuda())
    for name in ("conv1x1_bwd", "conv1x1_bwd_gated"):
        gxs = []

        def run(dw, acc, defer):
            gx = ops.new_act(B, 128, H, W, dtype, "cuda").zero_()
            if name == "conv1x1_bwd":
                ops.conv1x1_bwd(Slice(x2), Slice(g2, 64, 64), wd, Slice(gx), dw, accumulate=acc, defer=defer)
            else:
                ops.conv1x1_bwd_gated(Slice(x2), Slice(g2, 64, 64), wd, Slice(gx), dw, gate, 64, accumulate=acc, defer=defer)
            gxs.append(_sha(gx.view(torch.int16)))
        for form, h in _three_forms(run, (64, 128, 1, 1), 60).items():
            d[f"{name}_{tag}_{form}_dw"] = h
        assert gxs[0] == gxs[1] == gxs[2]                    # dL/dx does not depend on what becomes of dw
        d[f"{name}_{tag}_gx"] = gxs[0]
    return d


GROUPS = ([("forward", s) for s in FWD_SHAPES] + [("pair", s) for s in PAIR_SHAPES] +
          [("wgrad", ("f32",) + s + (kern,)) for s, kern in WGRAD_F32] +
          [("wgrad", (dn,) + s + ("c8",)) for dn in ("bf16", "f16") for s in WGRAD_16])


def group_digests(kind, args):
    return {"forward": forward_digests, "pair": pair_digests, "wgrad": wgrad_digests}[kind](*args)


def group_id(kind, args):
    return kind + "_" + "_".join(str(a) for a in args)


def digests():
    """{group id: {case: sha256 of the raw little-endian bytes of the output, or a launch count}}."""
    return {group_id(k, a): group_digests(k, a) for k, a in GROUPS}


if __name__ == "__main__":
    with open(sys.argv[2], "w") as f:
        json.dump(tiling_table() if sys.argv[1] == "tiling" else digests(), f, indent=1, sort_keys=True)
        f.write("\n")
