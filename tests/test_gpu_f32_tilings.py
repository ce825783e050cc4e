"""The fp32 MFMA convs (csrc/conv_mfma_f32.hip) held to float64 element by element in EVERY tiling f32_tiling hands out -- 8 x 32
(T8, two pixel rows per wave), 4 x 32 (T4), 4 x 32 one workgroup per CU (SOLO) and 2 x 32 with the couts split over the waves
(SPLIT) -- as single launches and as pair grids, and the four tilings compared with each other bit for bit.
tests/test_gpu_rounding.py sees SPLIT (SOLO for 1x1) only; tests/test_gpu_conv_bits.py reaches all four but compares digests
with an earlier commit's, which holds a refactor still and says nothing about whether the bits are right.

One small image, the batch selects the tiling.  `base` is 3 images; image b of a batch of B is base[b % 3] * 2^(b // 3 - E), E
half the largest b // 3 (tests/conv_bits.expand): the residual, the accumulate-into operand and the gate's `inputs` are scaled
the same way, ch, sp and the mask operand are not.  A power-of-two scale is exact through an fp32 fma chain (|exponent| <= 27:
nothing under- or overflows), so every image of a batch is distinct -- a read from the wrong image shows -- and the result for
image b must equal the result for base[b % 3] RUN ALONE (B = 1: SPLIT, SOLO for 1x1) times that power of two, bit for bit.
The float64 reference and S are computed for the 3 base images and rescaled exactly.
  geometry A  13 x 70: 3 tile columns, the last 6 pixels wide; last tile rows of 5 of 8, 1 of 4, 1 of 2 rows; no block count
              is a multiple of 8 (the xcd_remap tails run).  B = 1, 12 (SPLIT; SOLO inside a pair bracket), 17 (SOLO), 65 (T8),
              107 (T4 for the chained conv and 5x5, T8 otherwise); pairs at B = 5 (cout-split pair of <= 256 workgroups, padded),
              8 (> 256, unpadded), 12, 17.
  geometry B  16 x 64: exact tiles, W % 4 == 0, every row on 16 bytes.  B = 1, 25 (SOLO), 97 (T8), 161 (T4 / T8); the plain and
              ReLU epilogues and the chained conv only.
Every case first asserts its tiling, asking codon_conv_tiling_f32 with the descriptor of the launch it makes
(tests/conv_bits.tiling_premise; the same premises on the CPU: tests/test_conv_tiling_table.py).

Assertions, per case (form or entry point, geometry, B):
  1. float64 per element, the first, a middle and the last image: tests/bounds.assert_rounded with the project's fp32 bound
     tau = 2^-20 (S + |additive operands|).  Chained: mid against conv_ref of x, out against the float64 1x1 of the kernel's OWN
     mid; the statistics against the kernel's own out (maxima exact, sums within 2^-20 of the absolute sum).  Gated: the
     emitted input against tests/cac_ref.apply, y against conv_ref of the kernel's own emitted input.  Outputs are NaN-prefilled
     (y0 for the accumulating epilogues), operands and outputs are channel slices at coff = 64 of NaN-filled wider buffers
     whose other channels must stay NaN; inputs must be unchanged.
  2. bits across tilings, EVERY image, on the device: y, mid, out, the emitted input, pool and partials (per row strip in
     fp32: the layout does not depend on the tiling) equal the single-image results times 2^(b // 3 - E).  A mismatch names
     image, channel, pixel, the tile row and column under the case's tiling, and both values.
  3. pair brackets: one launch, the bits of the two launches made outside the bracket (B = 12: SOLO against SPLIT).
  4. codon_conv2d_gated_fwd / _emit_fwd == codon_cac_apply_fwd then codon_conv2d_fwd, bit for bit, at B = 17, 65, 107.

Measured on an MI355X: max |got - ref| / S against float64 over all cases of a tiling, in units of 2^-24 (the bound is 16).
Every bit comparison held, and |got - ref| / S does not change under a power-of-two scale, so the tilings differ only by
which images each batch probes:
                 conv 5x5  3x3  1x1   chained mid  out   gated y   emitted input   statistics sums
  T8                  5.4  6.0  4.9           5.0  5.6       5.1             1.8               2.2
  T4                  5.4   --   --           5.3  5.6       4.2             1.7               2.2   (3x3, 1x1 never take T4)
  SOLO                5.4  6.0  4.9           5.0  5.6       5.1             1.8               2.2
  SPLIT               5.4  6.0   --           5.3  5.6       5.1             1.8               2.2   (1x1 never splits)
  pair grid, SOLO     6.5  4.6   --           5.0  5.2       5.8             1.7               2.2   (its own operands)
  pair grid, SPLIT    6.5  4.6   --           5.0  5.2       5.8             1.7               2.2
The channel and row-strip maxima of the statistics are exact.  All 103 cases take 5 s.  GPU only."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from codon_amd import _lib as L
from tests import cac_ref, conv_bits as CB
from tests.bounds import TAU_UNIT, assert_rounded, conv_ref, tau_of
from tests.test_gpu_rounding import COFF, FORMS, _dev, _rand, _variants

NAN = float("nan")
A_BATCHES = [1, 12, 17, 65, 107]
B_BATCHES = [1, 25, 97, 161]
PAIR_BATCHES = [5, 8, 12, 17]
APPLY_BATCHES = (17, 65, 107)
F32 = torch.float32


# ---- buffers ----
def _guard(t):
    """(n, C, H, W) device values -> channels [COFF, COFF + C) of a NaN-filled (n, COFF + C, H, W) buffer."""
    n, Ch, H, W = t.shape
    full = torch.full((n, COFF + Ch, H, W), NAN, device=t.device)
    full[:, COFF:] = t
    return full


def _blank(n, Ch, H, W, dev):
    return torch.full((n, COFF + Ch, H, W), NAN, device=dev)


def _written(buf, what):
    assert torch.isnan(buf[:, :COFF]).all(), f"{what}: channels outside the output slice were written"
    return buf[:, COFF:]


def _unchanged(what, *pairs):
    for buf, t in pairs:
        assert torch.isnan(buf[:, :COFF]).all() and torch.equal(buf[:, COFF:], t), f"{what}: an input was written"


def _batch(base, B, dev=None, imgs=None):
    """base: name -> ((3, ...) CPU tensor, scaled?) -> name -> the images `imgs` (default all) of the batch of B, on dev."""
    return {n: CB.expand(t.to(dev) if dev is not None else t, B, imgs, sc) for n, (t, sc) in base.items()}


def _launch(preps, dev, paired=False):
    """preps: (call, collect) pairs, every call ONE kernel launch -> (the collected {name: output} of each, the launches the
    pair bracket took or None)."""
    from codon_amd import ops
    n = None
    if paired:
        with ops.conv_pair(dev) as br:
            for call, _ in preps:
                call()
        n = br.launches
    else:
        for call, _ in preps:
            call()
    return [collect() for _, collect in preps], n


def _merged(dicts):
    out = {}
    for d in dicts:
        assert not set(d) & set(out)
        out.update(d)
    return out


# ---- the entry points ----
class _Entry:
    """One entry point on one geometry: base operands, prep(o, what) -> (call, collect) per launch, check64 (assertion 1),
    same (bit identities between the launches of one case), col_step (pixels per element of an output's last axis)."""
    col_step = {}

    def alone(self, dev):
        """name -> (3, C, h, w): every output for the three base images, each run as a batch of one."""
        if self._alone is None:
            runs = []
            for i in range(3):
                o = {n: t[i:i + 1].to(dev) for n, (t, _) in self.base.items()}
                runs.append(_merged(_launch(self.prep(o, f"{self.what} image {i} alone"), dev)[0]))
            self._alone = {n: torch.cat([r[n] for r in runs]) for n in runs[0]}
        return self._alone

    def same(self, got, o, B, what):
        pass


class _Conv(_Entry):
    def __init__(self, k, cin, cout, geo, names=None, salt=0):
        self.k, self.cin, self.cout, self.geo, self.names, self._alone = k, cin, cout, geo, names, None
        H, W = CB.GEOMETRY[geo]
        seed = 100 * k + cin + cout + (1000 if geo == "B" else 0) + 10000 * salt
        img = lambda c, s, scaled=True: (_rand((3, c, H, W), seed + s), scaled)
        self.base = {"x": img(cin, 0), "r": img(cout, 2), "m": img(cout, 3, False), "y0": img(cout, 4)}
        # a dgrad launch reads dL/dy of the forward conv cout_f = cin <- cin_f = cout: its weight is (cin, cout, k, k), and the
        # launch itself is cin -> cout as the forward one is (FORMS is closed under cin <-> cout)
        self.packs = [p for p in (L.PACK_FWD, L.PACK_DGRAD) if self._names(p)]
        self.w = {p: _rand((cout, cin, k, k) if p == L.PACK_FWD else (cin, cout, k, k), seed + 1,
                           (2.0 / (k * k * (cout if p == L.PACK_FWD else cin))) ** 0.5) for p in self.packs}
        self.what = f"conv{k}x{k} {cin}->{cout} {geo}"
        self._wp, self._ref = {}, {}

    def _names(self, pack):
        return [v[0] for v in _variants(pack, None, None, None) if self.names is None or v[0] in self.names]

    def premise(self, B, in_pair=0):
        return CB.tiling_premise(self.geo, B, self.k, self.cin, self.cout, 0, in_pair)

    def prep(self, o, what):
        from codon_amd import ops
        from codon_amd.ops import Slice
        k, cin, cout = self.k, self.cin, self.cout
        n, _, H, W = o["x"].shape
        dev = o["x"].device
        xb, rb, mb = _guard(o["x"]), _guard(o["r"]), _guard(o["m"])
        sl = {"r": Slice(rb, COFF, cout), "m": Slice(mb, COFF, cout)}
        preps = []
        for pack in self.packs:
            if pack not in self._wp:
                self._wp[pack] = ops.packed_weight(self.w[pack].to(dev), pack, F32)
            wp = self._wp[pack]
            for name, kw, _, _, init in _variants(pack, None, None, None):
                if name not in self._names(pack):
                    continue
                yb = _guard(o["y0"]) if init else _blank(n, cout, H, W, dev)

                def call(yb=yb, wp=wp, kw=kw):
                    ops.conv2d(Slice(xb, COFF, cin), wp, Slice(yb, COFF, cout), k, **kw(sl))

                def collect(yb=yb, name=name):
                    _unchanged(f"{what} {name}", (xb, o["x"]), (rb, o["r"]), (mb, o["m"]))
                    return {name: _written(yb, f"{what} {name}")}
                preps.append((call, collect))
        return preps

    def check64(self, o, sel, B, imgs, what, where):
        r, m, y0 = o["r"].double(), o["m"].double(), o["y0"].double()
        for pack in self.packs:
            if pack not in self._ref:                       # the 3 base images, once; rescaled exactly below
                self._ref[pack] = conv_ref(self.base["x"][0], self.w[pack], self.k, pack)
            ref, S = (CB.expand(t, B, imgs) for t in self._ref[pack])
            for name, _, epi, add, _ in _variants(pack, r, m, y0):
                if name in self._names(pack):
                    assert_rounded(sel[name], ref, tau_of(S, *add), F32, f"{what} {name}", epi=epi, S=S, where=where)


class _Chain(_Entry):
    """codon_conv_chain1x1_fwd: `mid+res` (mid materialised, with a residual), `st` (the statistics form with mid, partials at
    channel offset 64) and `st0` (the statistics form without mid, partials at offset 0)."""
    col_step = {"st/partials": CB.TILE_COLS, "st0/partials": CB.TILE_COLS}

    def __init__(self, geo, only=None, salt=0):
        self.geo, self.only, self._alone, self._ref, self._wp = geo, only or ("mid+res", "st", "st0"), None, None, None
        H, W = CB.GEOMETRY[geo]
        seed = 40 + (1000 if geo == "B" else 0) + 10000 * salt
        self.base = {"x": (_rand((3, 128, H, W), seed), True), "r": (_rand((3, 64, H, W), seed + 30), True)}
        self.w5 = _rand((128, 128, 5, 5), seed + 10, (2.0 / (25 * 128)) ** 0.5)
        self.w1 = _rand((64, 128, 1, 1), seed + 20, (2.0 / 64) ** 0.5)
        self.what = f"chain1x1 {geo}"

    def premise(self, B, in_pair=0):
        return CB.tiling_premise(self.geo, B, 5, 128, 128, 1, in_pair)

    def prep(self, o, what):
        from codon_amd import ops
        from codon_amd.ops import Slice
        n, _, H, W = o["x"].shape
        dev = o["x"].device
        if self._wp is None:
            self._wp = (ops.packed_weight(self.w5.to(dev), L.PACK_FWD, F32), ops.packed_weight(self.w1.to(dev), L.PACK_CHAIN1X1, F32))
        w5, w1 = self._wp
        xb, rb = _guard(o["x"]), _guard(o["r"])
        tx, nparts = (W + CB.TILE_COLS - 1) // CB.TILE_COLS, ops.cac_fused_parts(H, W, F32)
        assert nparts == H * tx, (nparts, H, tx)            # one {sum, max} per channel and row strip of 32 pixels
        preps = []
        for mode in self.only:
            mid = _blank(n, 128, H, W, dev) if mode != "st0" else None
            out = _blank(n, 64, H, W, dev)
            pool, part = torch.full((n, 2, H, W), NAN, device=dev), torch.full((n, nparts, 128, 2), NAN, device=dev)
            choff = 0 if mode == "st0" else 64

            def call(mode=mode, mid=mid, out=out, pool=pool, part=part, choff=choff):
                ops.conv_chain1x1(Slice(xb, COFF, 128), w5, w1, Slice(out, COFF, 64), mid=Slice(mid, COFF, 128) if mid is not None else None,
                                  residual=Slice(rb, COFF, 64) if mode == "mid+res" else None,
                                  stats=None if mode == "mid+res" else (pool, part, choff))

            def collect(mode=mode, mid=mid, out=out, pool=pool, part=part, choff=choff):
                w_ = f"{what} {mode}"
                _unchanged(w_, (xb, o["x"]), (rb, o["r"]))
                d = {f"{mode}/out": _written(out, w_ + " out")}
                if mid is not None:
                    d[f"{mode}/mid"] = _written(mid, w_ + " mid")
                if mode != "mid+res":
                    assert torch.isnan(part[:, :, 64 - choff:128 - choff]).all(), f"{w_}: partials of the other stream were written"
                    # (n, H tx, 64, {sum, max}) -> (n, 128, H, tx): channel 2 c + j, j = 0 the sum and 1 the maximum
                    d[f"{mode}/partials"] = part[:, :, choff:choff + 64].reshape(n, H, tx, 64, 2).permute(0, 3, 4, 1, 2).reshape(n, 128, H, tx)
                    d[f"{mode}/pool"] = pool
                return d
            preps.append((call, collect))
        return preps

    def same(self, got, o, B, what):
        if "st" in self.only and "st0" in self.only:         # the intermediate reaching memory or not changes no bit
            for name in ("out", "pool", "partials"):
                assert torch.equal(got[f"st/{name}"], got[f"st0/{name}"]), f"{what}: {name} differs with and without mid"
        if "st" in self.only and "mid+res" in self.only:
            assert torch.equal(got["st/mid"], got["mid+res/mid"]), f"{what}: mid differs between the statistics and the plain form"

    def check64(self, o, sel, B, imgs, what, where):
        if self._ref is None:
            self._ref = conv_ref(self.base["x"][0], self.w5, 5)
        ref5, S5 = (CB.expand(t, B, imgs) for t in self._ref)
        r = o["r"].double()
        for mode in self.only:
            if mode == "st0":
                continue                                    # its outputs are st's, bit for bit (same)
            w_ = f"{what} {mode}"
            mid = sel[f"{mode}/mid"]
            assert_rounded(mid, ref5, tau_of(S5), F32, w_ + " mid", epi=torch.relu, S=S5, where=where)
            ref1, S1 = conv_ref(mid, self.w1, 1)             # the 1x1 of the kernel's own mid
            if mode == "mid+res":
                assert_rounded(sel[f"{mode}/out"], ref1, tau_of(S1, r), F32, w_ + " out", epi=lambda a: a + r, S=S1, where=where)
                continue
            assert_rounded(sel[f"{mode}/out"], ref1, tau_of(S1), F32, w_ + " out", S=S1, where=where)
            # the statistics of the kernel's own out: per pixel {max, sum} over the 64 channels, per channel and row strip {sum, max}
            out, pool = sel[f"{mode}/out"].double(), sel[f"{mode}/pool"].double()
            n, _, H, W = out.shape
            tx = (W + CB.TILE_COLS - 1) // CB.TILE_COLS
            assert torch.equal(pool[:, 0], out.amax(1)), f"{w_}: the per-pixel channel maximum is not the maximum of out"
            Sp = out.abs().sum(1, keepdim=True)
            assert_rounded(pool[:, 1:2], out.sum(1, keepdim=True), TAU_UNIT * Sp, F32, w_ + " pool sum", S=Sp, where=where)
            part = sel[f"{mode}/partials"].double().reshape(n, 64, 2, H, tx)
            strips = lambda t, fill: F.pad(t, (0, tx * CB.TILE_COLS - W), value=fill).reshape(n, 64, H, tx, CB.TILE_COLS)
            assert torch.equal(part[:, :, 1], strips(out, float("-inf")).amax(-1)), f"{w_}: a row strip's maximum is not the maximum of out"
            Ss = strips(out.abs(), 0.0).sum(-1)
            assert_rounded(part[:, :, 0], strips(out, 0.0).sum(-1), TAU_UNIT * Ss, F32, w_ + " strip sums", S=Ss,
                           where=lambda i: where((i[0], i[1], i[2], i[3] * CB.TILE_COLS)))


class _Gated(_Entry):
    """codon_conv2d_gated_fwd (`relu`: with ReLU) and codon_conv2d_gated_emit_fwd (`emit`: plain, the gated input written out)."""

    def __init__(self, k, cin, geo, only=None, salt=0):
        self.k, self.cin, self.geo, self.only, self._alone, self._wp = k, cin, geo, only or ("relu", "emit"), None, None
        H, W = CB.GEOMETRY[geo]
        seed = 300 + 10 * k + cin + 10000 * salt
        self.base = {"pre": (_rand((3, cin, H, W), seed), True), "inp": (_rand((3, cin, H, W), seed + 1), True),
                     "ch": (torch.sigmoid(_rand((3, 64), seed + 2)), False), "sp": (torch.sigmoid(_rand((3, 1, H, W), seed + 3)), False)}
        self.w = _rand((64, cin, k, k), seed + 4, (2.0 / (k * k * 64)) ** 0.5)
        self.what = f"gated conv{k}x{k} {cin}->64 {geo}"

    def premise(self, B, in_pair=0):                        # the gated convs take the plain rule of their shape
        return CB.tiling_premise(self.geo, B, self.k, self.cin, 64, 0, in_pair)

    def _weight(self, dev):
        from codon_amd import ops
        if self._wp is None:
            self._wp = ops.packed_weight(self.w.to(dev), L.PACK_FWD, F32)
        return self._wp

    def prep(self, o, what):
        from codon_amd import ops
        from codon_amd.ops import Slice
        k, cin = self.k, self.cin
        n, _, H, W = o["pre"].shape
        dev = o["pre"].device
        wp = self._weight(dev)
        pb, ib, ch, sp = _guard(o["pre"]), _guard(o["inp"]), o["ch"].clone(), o["sp"].clone()
        preps = []
        for mode in self.only:
            y = _blank(n, 64, H, W, dev)
            xg = _blank(n, cin, H, W, dev) if mode == "emit" else None

            def call(mode=mode, y=y, xg=xg):
                ops.conv2d_gated(Slice(pb, COFF, cin), Slice(ib, COFF, cin), ch, sp, wp, Slice(y, COFF, 64), k,
                                 relu=mode == "relu", emit=Slice(xg, COFF, cin) if xg is not None else None)

            def collect(mode=mode, y=y, xg=xg):
                w_ = f"{what} {mode}"
                _unchanged(w_, (pb, o["pre"]), (ib, o["inp"]))
                assert torch.equal(ch, o["ch"]) and torch.equal(sp, o["sp"]), f"{w_}: a gate operand was written"
                d = {f"{mode}/y": _written(y, w_ + " y")}
                if xg is not None:
                    d[f"{mode}/x"] = _written(xg, w_ + " emitted input")
                return d
            preps.append((call, collect))
        return preps

    def same(self, got, o, B, what):
        """Assertion 4: == codon_cac_apply_fwd, then codon_conv2d_fwd of what it wrote."""
        if B not in APPLY_BATCHES:
            return
        from codon_amd import ops
        from codon_amd.ops import Slice
        k, cin = self.k, self.cin
        n, _, H, W = o["pre"].shape
        dev = o["pre"].device
        pb, ib = _guard(o["pre"]), _guard(o["inp"])
        oc = torch.full((n, 128, H, W), NAN, device=dev)
        second = COFF + 64 if cin == 128 else COFF           # cin = 64: both streams of the apply read the one slice
        ops.cac_apply(Slice(pb, COFF, 64), Slice(pb, second, 64), o["ch"], o["sp"], Slice(ib, COFF, 64), Slice(ib, second, 64),
                      Slice(oc, 0, 64), Slice(oc, 64, 64))
        if "emit" in self.only:
            assert torch.equal(oc[:, :cin], got["emit/x"]), f"{what}: the emitted input is not cac_apply's output"
        for mode in self.only:
            y = _blank(n, 64, H, W, dev)
            ops.conv2d(Slice(oc, 0, cin), self._weight(dev), Slice(y, COFF, 64), k, relu=mode == "relu")
            assert torch.equal(_written(y, what), got[f"{mode}/y"]), f"{what} {mode}: gated conv != cac_apply then conv2d"

    def check64(self, o, sel, B, imgs, what, where):
        rep = self.cin // 64
        if "emit" in self.only:
            refx, Sx = cac_ref.apply(o["pre"], o["ch"].repeat(1, rep), o["sp"], o["inp"])
            assert_rounded(sel["emit/x"], refx, TAU_UNIT * Sx, F32, what + " emitted input", S=Sx, where=where)
            xg = sel["emit/x"]                              # the kernel's own gated input
        else:
            xg = cac_ref.apply(o["pre"], o["ch"].repeat(1, rep), o["sp"], o["inp"])[0].float()
        ref, S = conv_ref(xg, self.w, self.k)
        for mode in self.only:
            assert_rounded(sel[f"{mode}/y"], ref, tau_of(S), F32, f"{what} {mode} y", epi=torch.relu if mode == "relu" else None,
                           S=S, where=where)


@functools.lru_cache(maxsize=None)
def _entry(kind, *args):
    return {"conv": _Conv, "chain": _Chain, "gated": _Gated}[kind](*args)


# ---- assertions 1 and 2 on the outputs of one batch ----
def _verify(entry, got, B, t, what, dev):
    """got: name -> (B, C, h, w) device outputs of the batch under tiling t (B = 3 with exponents 0: the base images alone)."""
    H, W = CB.GEOMETRY[entry.geo]
    imgs = CB.probe_images(B)
    where = lambda i: f"image {imgs[i[0]]}, {CB.tile_where(t, H, W, i[2], i[3])}"
    errors = []
    try:
        entry.check64(_batch(entry.base, B, None, imgs), {n: g[imgs].cpu() for n, g in got.items()}, B, imgs, what, where)
    except AssertionError as e:
        errors.append(f"assertion 1 (float64): {e}")
    alone = entry.alone(dev)
    for name, g in got.items():
        msg = CB.bits_mismatch(g, alone[name], B, t, H, W, f"{what} {name}", col_step=entry.col_step.get(name, 1))
        if msg:
            errors.append(f"assertion 2 (bits across tilings): {msg}")
    assert not errors, "\n".join(errors)


def _case(entry, B):
    dev = _dev()
    H, W = CB.GEOMETRY[entry.geo]
    t = entry.premise(B)
    what = f"{entry.what} {B}x{H}x{W} {CB.TILING_NAME[t]}"
    if B == 1:                                              # the three base images, each alone: a batch of 3 with exponents 0
        return _verify(entry, entry.alone(dev), 3, t, what, dev)
    o = _batch(entry.base, B, dev)
    got = _merged(_launch(entry.prep(o, what), dev)[0])
    entry.same(got, o, B, what)
    _verify(entry, got, B, t, what, dev)


_ids = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)
_GEO_BATCHES = [("A", b) for b in A_BATCHES] + [("B", b) for b in B_BATCHES]


@pytest.mark.parametrize("geo,B", _GEO_BATCHES, ids=lambda v: str(v))
@pytest.mark.parametrize("form", FORMS, ids=_ids)
def test_conv2d_every_tiling(form, geo, B):
    """Geometry A: the three forward and the four dgrad epilogues; geometry B: plain and ReLU."""
    _case(_entry("conv", *form, geo, None if geo == "A" else ("plain", "relu")), B)


@pytest.mark.parametrize("geo,B", _GEO_BATCHES, ids=lambda v: str(v))
def test_chain1x1_every_tiling(geo, B):
    _case(_entry("chain", geo), B)


@pytest.mark.parametrize("B", A_BATCHES)
@pytest.mark.parametrize("k,cin", [(k, ci) for k, ci, _ in CB.GATED_FORMS], ids=lambda v: str(v))
def test_gated_every_tiling(k, cin, B):
    _case(_entry("gated", k, cin, "A"), B)


PAIRS = {"conv5x5": lambda s: _entry("conv", 5, 64, 64, "A", ("relu",), s),
         "conv3x3": lambda s: _entry("conv", 3, 64, 64, "A", ("relu",), s),
         "chain_stats": lambda s: _entry("chain", "A", ("st",), s),
         "gated5x5_emit": lambda s: _entry("gated", 5, 64, "A", ("emit",), s)}


@pytest.mark.parametrize("B", PAIR_BATCHES)
@pytest.mark.parametrize("kind", sorted(PAIRS))
def test_pair_bracket_every_tiling(kind, B):
    """Two convs of one shape on their own operands inside ops.conv_pair: ONE launch, the bits of the two launches made
    outside the bracket (assertion 3), and assertions 1 and 2 on what the pair grid wrote."""
    dev = _dev()
    ents = [PAIRS[kind](s) for s in (1, 2)]
    H, W = CB.GEOMETRY["A"]
    t_in, t_out = ents[0].premise(B, 1), ents[0].premise(B, 0)
    what = f"pair of {ents[0].what} {B}x{H}x{W} {CB.TILING_NAME[t_in]}"
    os_ = [_batch(e.base, B, dev) for e in ents]
    preps = lambda: [p for e, o, tag in zip(ents, os_, "ab") for p in e.prep(o, f"{what} conv {tag}")]
    inside, n = _launch(preps(), dev, paired=True)
    assert n == 1, f"{what}: the bracket took {n} launches"
    outside, _ = _launch(preps(), dev)
    for tag, gi, go in zip("ab", inside, outside):
        for name in gi:
            assert torch.equal(gi[name], go[name]), (f"{what} conv {tag} {name}: the pair grid ({CB.TILING_NAME[t_in]}) and the "
                                                     f"launch outside the bracket ({CB.TILING_NAME[t_out]}) differ")
    for tag, e, gi in zip("ab", ents, inside):
        _verify(e, gi, B, t_in, f"{what} conv {tag}", dev)
