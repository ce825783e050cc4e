"""The CAC gate, forward and backward, in float64 on the CPU (test infrastructure; no GPU, no codon_amd import): the plain
restatement of the headers of codon_amd/csrc/cac.hip and cac_bwd.hip.  Every function returns (ref, S): ref the value
and S the SAME expression over absolute values (an operand that is itself a computed quantity enters with its own S), so
that |kernel - ref| <= 2^-20 S is the project's per-element bound (tests/bounds.py).

Forward (Fcat = [pre_c | pre]: colour channels 0..63, depth channels 64..127):
  stats   per pixel : chmax = max_c Fcat, chmean = sum_c Fcat / 128        (pooled planes 0 and 1)
          per tile  : {sum, max} of every channel over `tile` consecutive pixels of the flattened plane
  gate    pools = {sum of the tile sums / HW, max of the tile maxima}; a = b1 + w1 pool (both pools), hid = relu(a),
          z = (b2 + w2 hid_avg) + (b2 + w2 hid_max), ch = sigmoid(z)
  spatial logits = conv5x5_{2->1, pad 2}(pooled), sp = sigmoid(logits)
  apply   out = pre ch sp + inputs

Backward: the analytic expressions of cac_bwd.hip's header, evaluated on the operands THE KERNEL IS GIVEN (g_out, g_out_c,
pre, pre_c and the forward's saved ch, sp, pooled, pools) -- never autograd through a re-run forward.  Routing as the kernel
states it: the global max-pool's gradient goes to the FIRST pixel equal to pools[:, 1]; the channel max's to the FIRST
channel, in Fcat order, equal to pooled[:, 0].  Equality is between fp32 numbers the forward produced, so it is exact."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def _d(t):
    return t.detach().cpu().double()


def fcat(pre_c, pre):
    return torch.cat((_d(pre_c), _d(pre)), 1)


def stats(pre_c, pre, tile: int, chs=None):
    """pre_c, pre: (B, 64, H, W).  chs (optional, (B, 64)): cac_stats_scaled -- every value of channel c is first multiplied
    by chs[b][c & 63] and ROUNDED TO fp32 (one fp32 multiply: the maxima are maxima of those products).
    ref / S keys: chmax, chmean (B, H, W); tile_sum, tile_max (B, ntiles, 128)."""
    X = fcat(pre_c, pre)
    B, _, H, W = X.shape
    if chs is not None:
        g = _d(chs).repeat(1, 2)[:, :, None, None]
        prod = X * g                                   # exact in float64 (24 + 24 bits)
        Xm, X = prod.float().double(), prod            # the maxima see the fp32 product, the sums any rounding of it
        A = prod.abs()
    else:
        Xm, A = X, X.abs()
    HW = H * W
    nt = (HW + tile - 1) // tile
    pad = nt * tile - HW
    flat = lambda t, fill: F.pad(t.reshape(B, 128, HW), (0, pad), value=fill).reshape(B, 128, nt, tile)
    ref = {"chmax": Xm.max(1)[0], "chmean": X.sum(1) / 128,
           "tile_sum": flat(X, 0.0).sum(3).transpose(1, 2), "tile_max": flat(Xm, float("-inf")).max(3)[0].transpose(1, 2)}
    S = {"chmax": ref["chmax"].abs(), "chmean": A.sum(1) / 128,
         "tile_sum": flat(A, 0.0).sum(3).transpose(1, 2), "tile_max": ref["tile_max"].abs()}
    return ref, S


def pools_of(partials, HW: int):
    """partials: (B, ntiles, 128, 2) per-tile {sum, max} -> pools (B, 2, 128) = {mean over H W, max}."""
    p = _d(partials)
    ref = torch.stack((p[..., 0].sum(1) / HW, p[..., 1].max(1)[0]), 1)
    S = torch.stack((p[..., 0].abs().sum(1) / HW, ref[:, 1].abs()), 1)
    return ref, S


def mlp(pools, w1, b1, w2, b2):
    """pools (B, 2, 128) -> ref / S keys: a (B, 2, 8) hidden pre-activations, z (B, 64) logits, ch (B, 64).
    S['z'] = |w2| relu-propagated (|w1| |pool| + |b1|) + |b2| over both branches; S['ch'] = S['z'] / 4 (the sigmoid's slope)."""
    p, w1, b1, w2, b2 = _d(pools), _d(w1), _d(b1), _d(w2), _d(b2)
    a = p @ w1.t() + b1                                # (B, 2, 8)
    Sa = p.abs() @ w1.abs().t() + b1.abs()
    zb = torch.relu(a) @ w2.t() + b2                   # (B, 2, 64)
    Szb = Sa @ w2.abs().t() + b2.abs()
    z = zb[:, 0] + zb[:, 1]
    Sz = Szb[:, 0] + Szb[:, 1]
    return {"a": a, "z": z, "ch": torch.sigmoid(z)}, {"a": Sa, "z": Sz, "ch": Sz / 4}


def gate(partials_or_Fcat, w1, b1, w2, b2, HW: int = None):
    """The pools {mean, max} -- from (B, ntiles, 128, 2) partials (HW given) or from Fcat (B, 128, H, W) -- then mlp().
    ref / S keys: pools, a, z, ch."""
    t = _d(partials_or_Fcat)
    if HW is not None:
        pools, Sp = pools_of(t, HW)
    else:
        pools = torch.stack((t.mean((2, 3)), t.amax((2, 3))), 1)
        Sp = torch.stack((t.abs().mean((2, 3)), pools[:, 1].abs()), 1)
    ref, S = mlp(pools, w1, b1, w2, b2)
    ref["pools"], S["pools"] = pools, Sp
    return ref, S


def spatial(pooled, ws):
    """pooled (B, 2, H, W) = {chmax, chmean}, ws (1, 2, 5, 5) -> ref / S keys: logits, sp (B, 1, H, W)."""
    p, w = _d(pooled), _d(ws)
    z = F.conv2d(p, w, None, 1, 2)
    Sz = F.conv2d(p.abs(), w.abs(), None, 1, 2)
    return {"logits": z, "sp": torch.sigmoid(z)}, {"logits": Sz, "sp": Sz / 4}


def apply(pre, ch, sp, inputs):
    """pre, inputs (B, 64, H, W), ch (B, 64), sp (B, 1, H, W) -> (pre ch sp + inputs, |pre ch sp| + |inputs|)."""
    t = _d(pre) * _d(ch)[:, :, None, None] * _d(sp)
    return t + _d(inputs), t.abs() + _d(inputs).abs()


def sq_scale(x, ch):
    """ew_sq_scale: y = x x ch[b][c]."""
    t = _d(x) ** 2 * _d(ch)[:, :, None, None]
    return t, t.abs()


def first_pixel(X, pools_max):
    """(B, 128) index of the first pixel of the flattened plane equal to pools_max, -1 where none is."""
    B, Cc, H, W = X.shape
    eq = X.reshape(B, Cc, H * W) == _d(pools_max)[:, :, None]
    idx = eq.double().argmax(2)                        # argmax of a 0/1 tensor: the first 1
    return torch.where(eq.any(2), idx, torch.full_like(idx, -1))


def first_channel(X, chmax):
    """(B, H, W) index of the first channel, in Fcat order, equal to chmax, -1 where none is."""
    eq = X == _d(chmax)[:, None]
    idx = eq.double().argmax(1)
    return torch.where(eq.any(1), idx, torch.full_like(idx, -1))


def backward(g_out, g_out_c, pre, pre_c, ch, sp, pooled, pools, w1, b1, w2, ws, argpix=None, argch=None):
    """ref / S keys: g_pre, g_pre_c (B, 64, H, W), dw1 (8, 128), db1 (8), dw2 (64, 8), db2 (64), dws (1, 2, 5, 5); also the
    intermediates g_z, g_ch, gs, a, g_pools, g_pooled and the routes argpix (B, 128), argch (B, H, W).
    argpix / argch (optional) OVERRIDE the routing: the sensitivity tests send a maximum to the second tied element."""
    X = fcat(pre_c, pre)
    G = fcat(g_out_c, g_out)
    B, _, H, W = X.shape
    HW = H * W
    ch, sp, pooled, pools = _d(ch), _d(sp), _d(pooled), _d(pools)
    w1, b1, w2, ws = _d(w1), _d(b1), _d(w2), _d(ws)
    ch4 = ch[:, :, None, None]
    # dL/dch and dL/dsp: gg = g_out pre + g_out_c pre_c per depth/colour channel pair
    gg = G[:, 64:] * X[:, 64:] + G[:, :64] * X[:, :64]
    Sgg = G[:, 64:].abs() * X[:, 64:].abs() + G[:, :64].abs() * X[:, :64].abs()
    g_ch, S_gch = (gg * sp).sum((2, 3)), (Sgg * sp.abs()).sum((2, 3))
    g_sp, S_gsp = (gg * ch4).sum(1, keepdim=True), (Sgg * ch4.abs()).sum(1, keepdim=True)
    g_z, S_gz = g_sp * sp * (1 - sp), S_gsp * sp.abs() * (1 + sp.abs())            # sigmoid'
    gs, S_gs = g_ch * ch * (1 - ch), S_gch * ch.abs() * (1 + ch.abs())
    # MLP backward (shared weights, both pools)
    a = pools @ w1.t() + b1                                                         # (B, 2, 8)
    S_a = pools.abs() @ w1.abs().t() + b1.abs()
    on = (a > 0).double()
    hid, S_hid = torch.relu(a), S_a * on
    ghid = (gs @ w2)[:, None, :] * on                                               # (B, 2, 8)
    S_ghid = (S_gs @ w2.abs())[:, None, :] * on
    g_pools, S_gpools = ghid @ w1, S_ghid @ w1.abs()                                # (B, 2, 128): d avg, d max
    dw1 = torch.einsum("bpj,bpk->jk", ghid, pools)
    S_dw1 = torch.einsum("bpj,bpk->jk", S_ghid, pools.abs())
    db1, S_db1 = ghid.sum((0, 1)), S_ghid.sum((0, 1))
    dw2 = torch.einsum("bo,bj->oj", gs, hid[:, 0] + hid[:, 1])
    S_dw2 = torch.einsum("bo,bj->oj", S_gs, S_hid[:, 0] + S_hid[:, 1])
    db2, S_db2 = 2 * gs.sum(0), 2 * S_gs.sum(0)
    # spatial gate backward: transposed 5x5 and its weight gradient
    g_pooled, S_gpooled = F.conv_transpose2d(g_z, ws, None, 1, 2), F.conv_transpose2d(S_gz, ws.abs(), None, 1, 2)
    cw = lambda p, g: torch.nn.grad.conv2d_weight(p, (1, 2, 5, 5), g, stride=1, padding=2)
    dws, S_dws = cw(pooled, g_z), cw(pooled.abs(), S_gz)
    # dL/dFcat: direct + avg-pool broadcast + channel-mean broadcast + the two routed maxima
    ch128 = torch.cat((ch, ch), 1)[:, :, None, None]
    gF = G * ch128 * sp + g_pools[:, 0, :, None, None] / HW + g_pooled[:, 1:2] / 128
    S_gF = G.abs() * ch128.abs() * sp.abs() + S_gpools[:, 0, :, None, None] / HW + S_gpooled[:, 1:2] / 128
    argpix = first_pixel(X, pools[:, 1]) if argpix is None else argpix
    argch = first_channel(X, pooled[:, 0]) if argch is None else argch
    hit_p = (torch.arange(HW)[None, None, :] == argpix[:, :, None]).reshape(B, 128, H, W).double()
    hit_c = (torch.arange(128)[None, :, None, None] == argch[:, None]).double()
    gF = gF + hit_p * g_pools[:, 1, :, None, None] + hit_c * g_pooled[:, 0:1]
    S_gF = S_gF + hit_p * S_gpools[:, 1, :, None, None] + hit_c * S_gpooled[:, 0:1]
    ref = {"g_pre": gF[:, 64:], "g_pre_c": gF[:, :64], "dw1": dw1, "db1": db1, "dw2": dw2, "db2": db2, "dws": dws,
           "g_z": g_z, "g_ch": g_ch, "gs": gs, "a": a, "g_pools": g_pools, "g_pooled": g_pooled, "argpix": argpix, "argch": argch}
    S = {"g_pre": S_gF[:, 64:], "g_pre_c": S_gF[:, :64], "dw1": S_dw1, "db1": S_db1, "dw2": S_dw2, "db2": S_db2, "dws": S_dws,
         "g_z": S_gz, "g_ch": S_gch, "gs": S_gs, "a": S_a, "g_pools": S_gpools, "g_pooled": S_gpooled}
    return ref, S
