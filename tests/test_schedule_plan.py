"""The schedule of a CODONNet forward as a value (codon_amd.model.plan_forward): the cases DESIGN documents, the
implications the executor relies on, and equality with the inline expressions the plan was moved out of.  CPU only: the
planner makes no library call."""
import itertools
import types

import pytest
import torch

from codon_amd import _lib as L
from codon_amd import model as M

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
FIELDS = ("fused_stats", "gated", "emit16", "pairs", "two", "tail")

# dense around every threshold of the plan: 8 x 32 and 4 x 32 tiles (256, 383, 4096), 32 768 pixels, 2**21 pixels
BS = (1, 2, 3, 4, 5, 8, 16, 32, 50, 88)
HS = (1, 5, 8, 31, 32, 37, 64, 96, 127, 128, 181, 182, 256, 370, 480, 1024)
WS = (1, 3, 31, 32, 33, 62, 64, 96, 126, 128, 180, 181, 256, 463, 640, 2048)
SHAPES = tuple(itertools.product(BS, HS, WS))
FLAGS = tuple(itertools.product((False, True), repeat=3))          # keep, split5, profiling

SWITCHES = {
    "default": {},
    "no_gated16": dict(GATED_16BIT=False),
    "no_emit": dict(GATED_EMIT=False),
    "one_stream": dict(TWO_STREAMS=False),
    "no_tail": dict(CAC_TAIL=False),
    "no_fused_f32": dict(FUSED_STATS_F32=False),
    "no_pairs": dict(PAIR_MAX16=0, PAIR_MAX32=0),
    "no_pairs_wide_two": dict(PAIR_MAX16=0, PAIR_MAX32=0, TWO_STREAMS_MAX16=4096, TWO_STREAMS_MAX32=4096),
    "wide_pairs": dict(PAIR_MAX16=1 << 20, PAIR_MAX32=4096),
    "no_two_grid": dict(TWO_STREAMS_MAX16=0, TWO_STREAMS_MAX32=0, PAIR_MAX16=100, PAIR_MAX32=100),
}


def _set(monkeypatch, name):
    for k, v in SWITCHES[name].items():
        monkeypatch.setattr(M, k, v)


def _plan(B, H, W, adt, keep=False, split5=False, profiling=False, on_gpu=True):
    return M.plan_forward(B, H, W, adt, keep, split5, profiling, on_gpu)


# ---- 1. the documented cases, default switches ------------------------------------------------------------------------

def test_plan_is_a_frozen_value_with_the_six_fields():
    p = _plan(1, 128, 128, F32)
    assert isinstance(p, M.ForwardPlan) and p._fields == FIELDS
    with pytest.raises(AttributeError):
        p.pairs = False
    assert p == _plan(1, 128, 128, F32) and "pairs=True" in repr(p)


def test_one_small_fp32_image():
    p = _plan(1, 128, 128, F32)
    assert p.pairs and p.fused_stats and p.tail and p.gated and p.emit16 and not p.two


def test_one_fp16_image_of_the_reference_script():
    p = _plan(1, 370, 463, F16)
    assert p.pairs and p.fused_stats and p.tail and p.gated and p.emit16


def test_full_batch_fp32_inference():
    p = _plan(32, 480, 640, F32)
    assert not p.pairs and not p.two and not p.fused_stats and p.gated


def test_full_batch_bf16_inference():
    p = _plan(32, 480, 640, BF16)
    assert 32 * 480 * 640 > M.CAC_TAIL_MAX_PIXELS == 1 << 21
    assert p.fused_stats and not p.tail and not p.pairs


@pytest.mark.parametrize("shape", [(2, 64, 96), (4, 128, 128), (32, 480, 640)])
def test_fp32_training(shape):
    p = _plan(*shape, F32, keep=True)
    assert not p.gated and not p.pairs and not p.two


@pytest.mark.parametrize("shape", [(2, 64, 96), (4, 128, 128), (32, 480, 640)])
def test_bf16_training(shape):
    p = _plan(*shape, BF16, keep=True)
    assert p.gated and p.emit16


@pytest.mark.parametrize("shape", [(1, 128, 128), (32, 480, 640)])
def test_f16x3(shape):
    p = _plan(*shape, F32, split5=True)
    assert not p.gated and not p.emit16 and not p.fused_stats


# ---- 2. properties over the grid --------------------------------------------------------------------------------------

@pytest.mark.parametrize("switches", list(SWITCHES))
def test_implications(monkeypatch, switches):
    _set(monkeypatch, switches)
    n = 0
    for (B, H, W), adt, (keep, split5, profiling), on_gpu in itertools.product(SHAPES, DTYPES, FLAGS, (True, False)):
        p = M.plan_forward(B, H, W, adt, keep, split5, profiling, on_gpu)
        where = (switches, B, H, W, adt, keep, split5, profiling, on_gpu, p)
        assert not (p.pairs and p.two), where
        assert not (keep and (p.pairs or p.two)), where
        assert not (profiling and p.pairs), where
        assert p.gated or not p.emit16, where
        assert on_gpu or not p.two, where
        n += 1
    assert n == len(SHAPES) * 3 * 8 * 2


@pytest.mark.parametrize("switches", list(SWITCHES))
def test_fp32_statistics_do_not_depend_on_the_batch(monkeypatch, switches):
    """whether an fp32 image's CAC statistics are fused, and whether the one-launch gate folds them, is chosen by
    H x W only -- an image's bits do not depend on the batch it arrives in."""
    _set(monkeypatch, switches)
    for H, W, (keep, split5, profiling) in itertools.product(HS, WS, FLAGS):
        seen = {(p.fused_stats, p.tail) for p in (M.plan_forward(B, H, W, F32, keep, split5, profiling, True) for B in BS)}
        assert len(seen) == 1, (switches, H, W, keep, split5, profiling, seen)


def test_two_streams_need_profiling_or_a_switch(monkeypatch):
    """With the default switches every grid small enough for the two-stream schedule is small enough to pair."""
    for (B, H, W), adt, keep, split5 in itertools.product(SHAPES, DTYPES, (False, True), (False, True)):
        assert not M.plan_forward(B, H, W, adt, keep, split5, False, True).two, (B, H, W, adt, keep, split5)
    assert _plan(1, 128, 128, F32, profiling=True).two and _plan(1, 128, 128, BF16, profiling=True).two
    _set(monkeypatch, "no_pairs")
    assert _plan(1, 128, 128, F32).two and _plan(1, 128, 128, BF16).two
    assert not _plan(1, 128, 128, F32).pairs and not _plan(1, 128, 128, F32, on_gpu=False).two


# ---- 3. the expressions the plan was moved out of ---------------------------------------------------------------------

def _stats_tiles(H, W):
    """codon_cac_stats_tiles (csrc/cac.hip): 256-pixel tiles up to 32 768 pixels, 2048-pixel tiles above."""
    return (H * W + 255) // 256 if H * W <= 32768 else (H * W + 2047) // 2048


def _inline_plan(B, H, W, adt, keep, split5, profile, dev):
    """The schedule expressions of _CODONBase._forward_impl at commit c6e6acd (codon_amd/model.py:792-891), verbatim, in
    the order they stood there.  Stand-ins for what they read: the module switches, ops.is_c8 / ops.PROFILE, the tile
    count `nt` of the statistics pass (the fused count is not read by any of them)."""
    (GATED_16BIT, GATED_EMIT, TWO_STREAMS, TWO_STREAMS_MAX32, TWO_STREAMS_MAX16, PAIR_MAX16, PAIR_MAX32, CAC_TAIL,
     FUSED_STATS_F32, CAC_TAIL_MAX_PIXELS) = (
        M.GATED_16BIT, M.GATED_EMIT, M.TWO_STREAMS, M.TWO_STREAMS_MAX32, M.TWO_STREAMS_MAX16, M.PAIR_MAX16, M.PAIR_MAX32,
        M.CAC_TAIL, M.FUSED_STATS_F32, M.CAC_TAIL_MAX_PIXELS)
    ops = types.SimpleNamespace(is_c8=lambda dt: dt in (torch.bfloat16, torch.float16), PROFILE=profile,
                                cac_fused_parts=lambda H, W, adt: None, cac_stats_tiles=_stats_tiles)

    fused_stats = ops.is_c8(adt) or (FUSED_STATS_F32 and CAC_TAIL and adt == torch.float32 and not split5 and H * W <= 32768)

    emit16 = GATED_EMIT and not split5 and ((ops.is_c8(adt) and GATED_16BIT) or (adt == torch.float32 and not keep))
    gated = not split5 and (((not keep) and (adt == torch.float32 or GATED_16BIT)) or (keep and emit16))

    emit16 = emit16 and gated

    pairs = (not keep) and ops.PROFILE is None and \
        B * ((H + 7) // 8) * ((W + 31) // 32) <= (PAIR_MAX16 if ops.is_c8(adt) else min(PAIR_MAX32, 383))

    two = TWO_STREAMS and (not keep) and (not pairs) and dev.type == "cuda" and (
        B * ((H + 7) // 8) * ((W + 31) // 32) <= TWO_STREAMS_MAX16 if ops.is_c8(adt) else
        B * ((H + 3) // 4) * ((W + 31) // 32) <= TWO_STREAMS_MAX32)

    nt = ops.cac_fused_parts(H, W, adt) if fused_stats else ops.cac_stats_tiles(H, W)

    tail = CAC_TAIL and ((B * H * W <= CAC_TAIL_MAX_PIXELS or adt == torch.float32) if fused_stats
                         else (nt <= L.CAC_FOLDS or H * W <= 32768))
    return fused_stats, gated, emit16, pairs, two, tail


@pytest.mark.parametrize("switches", list(SWITCHES))
def test_plan_equals_the_inline_expressions_it_replaced(monkeypatch, switches):
    _set(monkeypatch, switches)
    devs = {True: types.SimpleNamespace(type="cuda"), False: types.SimpleNamespace(type="cpu")}
    n = 0
    for (B, H, W), adt, (keep, split5, profiling), on_gpu in itertools.product(SHAPES, DTYPES, FLAGS, (True, False)):
        want = _inline_plan(B, H, W, adt, keep, split5, {"key": None} if profiling else None, devs[on_gpu])
        got = M.plan_forward(B, H, W, adt, keep, split5, profiling, on_gpu)
        assert tuple(bool(v) for v in got) == tuple(bool(v) for v in want), (switches, B, H, W, adt, keep, split5, profiling, on_gpu)
        n += 1
    assert n == len(SHAPES) * 3 * 8 * 2          # every shape of the grid, with every dtype and flag


def test_forward_impl_reads_the_schedule_from_the_plan_only():
    """No schedule switch is read by the executor itself."""
    import inspect
    src = inspect.getsource(M._CODONBase._forward_impl)
    assert src.count("plan_forward(") == 1
    for name in ("GATED_16BIT", "GATED_EMIT", "TWO_STREAMS", "PAIR_MAX", "CAC_TAIL", "FUSED_STATS_F32"):
        assert name not in src, name
