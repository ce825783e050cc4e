"""The hole-aware L1 + SSIM loss and the label plane on the MI355X.  The yardstick is the float64 torch
restatement in tests/masked_loss_ref.py (pinned on the CPU by tests/test_masked_loss_cpu.py); the labeled crops are held to
equal bits with tests/train_data_labeled_ref.py.  Bars: value 2e-6 and gradient 1e-4 relative are the ones
test_l1_ssim_loss_forward_backward holds the unmasked loss to; 1e-6 / 2e-5 for shards are grad_equality_selfcheck's."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from codon_amd import io, train
from tests import masked_loss_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- inputs --------------------------------------------------------------------------------------------------------------------

def _mask(g, H, W):
    """Isolated holes (3 %) and a few rectangular blobs; at least 25 % of the pixels stay valid."""
    v = g.uniform(size=(H, W)) > 0.03
    for _ in range(3):
        h, w = int(g.integers(2, max(3, H // 4))), int(g.integers(2, max(3, W // 4)))
        y, x = int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1))
        v[y:y + h, x:x + w] = False
    assert v.mean() >= 0.25
    return v


def _case(B, H, W, seed=0, special=True):
    """p, t, v as numpy (float64, float64, bool).  With special and B >= 5: image B-2 has e_b = 0 but n_b > 0 (a hole every
    fifth pixel both ways: every 13x13 window holds one), image B-1 has n_b = 0."""
    g = np.random.default_rng(seed)
    p = g.uniform(0, 1, (B, 1, H, W)).astype(np.float32).astype(np.float64)
    t = np.clip(p + g.normal(0, 0.1, p.shape), 0.01, 1).astype(np.float32).astype(np.float64)
    v = np.stack([_mask(g, H, W) for _ in range(B)])[:, None]
    if special and B >= 5:
        v[B - 2] = True
        v[B - 2, 0, ::5, ::5] = False
        v[B - 1] = False
    return p, t, v


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _run(p, t, v, w=(1.0, 0.7), explicit=True, up=None):
    """The HIP loss and its gradient: (loss tensor (), grad tensor) on the device."""
    from codon_amd.metrics import MaskedL1SSIMLoss
    pd = (p if torch.is_tensor(p) else _dev(p)).clone().requires_grad_(True)
    td = t if torch.is_tensor(t) else _dev(t)
    vd = None if not explicit else (v if torch.is_tensor(v) else _dev(v, torch.uint8))
    loss = MaskedL1SSIMLoss(*w)(pd, td, vd)
    (loss if up is None else loss * up).backward()
    return loss.detach(), pd.grad


def _ref(p, t, v, w=(1.0, 0.7)):
    pt = torch.from_numpy(p).requires_grad_(True)
    loss = M.masked_loss(pt, torch.from_numpy(t), torch.from_numpy(v), *w)
    loss.backward()
    return float(loss.detach()), pt.grad


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


# ---- value and gradient against the float64 restatement ------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W", [(1, 37, 53), (5, 37, 53), (1, 128, 128), (5, 128, 128), (1, 370, 463)])
def test_value_and_gradient_match_float64(B, H, W):
    from codon_amd import metrics
    p, t, v = _case(B, H, W, seed=H + B)
    ref, gref = _ref(p, t, v)
    loss, grad = _run(p, t, v)
    dl = abs(float(loss) - ref)
    rel = float((grad.cpu().double() - gref).norm() / gref.norm())
    print(f"masked loss {B}x{H}x{W}: |dloss| {dl:.3e} (bar 2e-6)  grad rel {rel:.3e} (bar 1e-4)  loss {ref:.6f}")
    assert dl < 2e-6 and rel < 1e-4
    want = M.counts(torch.from_numpy(t), torch.from_numpy(v)).numpy()
    got = metrics.masked_counts(_dev(t), _dev(v, torch.uint8)).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    if H * W <= 37 * 53:
        assert np.array_equal(got, M.counts_brute(t, v))
    if B >= 5:
        assert want[B - 2, 1] == 0 and want[B - 2, 0] > 0 and want[B - 1].tolist() == [0, 0]
        assert not grad[B - 1].any() and grad[B - 2].any()                      # n_b = 0: an all-zero gradient


def test_empty_images_contribute_what_the_definition_says():
    """n_b = 0: 0 loss, zero gradient.  e_b = 0: the L1 term alone.  Checked on single images, where the loss IS the term."""
    p, t, v = _case(5, 37, 53, seed=2)
    loss, grad = _run(p[4:], t[4:], v[4:])
    assert float(loss) == 0.0 and not grad.any() and _bits(grad).eq(0).all()
    loss, grad = _run(p[3:4], t[3:4], v[3:4], w=(1.0, 0.7))
    l1 = float(np.abs(p[3] - t[3])[v[3]].mean())
    print(f"e_b = 0 image: loss {float(loss):.8f}, its L1 term {l1:.8f}")
    assert abs(float(loss) - l1) < 2e-6
    gl1 = np.where(v[3:4], np.sign(p[3:4] - t[3:4]) / v[3].sum(), 0.0)
    assert float((grad.cpu().double() - torch.from_numpy(gl1)).norm() / np.linalg.norm(gl1)) < 1e-6


# ---- nothing in a hole reaches anything ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W", [(5, 37, 53), (1, 128, 128)])
def test_hole_invariance_bit_for_bit(B, H, W):
    p, t, v = _case(B, H, W, seed=7)
    vd = _dev(v, torch.uint8)
    hole = ~vd.bool()
    loss0, grad0 = _run(p, t, vd)
    assert torch.isfinite(loss0) and torch.isfinite(grad0).all()
    assert _bits(grad0)[hole.cpu()].eq(0).all()                                 # exactly +0.0 (not -0.0) at every invalid pixel
    for jp, jt in ((0.25, 3.0), (-1e30, 1e30), (float("nan"), float("nan")), (float("inf"), -float("inf")),
                   (-float("inf"), float("nan"))):
        pd, td = _dev(p), _dev(t)
        pd[hole], td[hole] = jp, jt
        for up in (None, -2.0):                                                 # a negative upstream gradient must not leave -0.0
            loss, grad = _run(pd, td, vd, up=up)
            assert torch.equal(_bits(loss), _bits(loss0)), (jp, jt)
            assert not torch.isnan(grad).any() and _bits(grad)[hole.cpu()].eq(0).all(), (jp, jt, up)
            want = grad0 if up is None else torch.where(hole, torch.zeros_like(grad0), grad0 * up)     # * -2 is exact
            assert torch.equal(_bits(grad), _bits(want)), (jp, jt, up)


def test_default_validity_is_target_nonzero():
    from codon_amd import metrics
    p, t, v = _case(5, 37, 53, seed=8)
    t0 = np.where(v, t, 0.0)
    la, ga = _run(p, t0, v, explicit=False)
    lb, gb = _run(p, t0, t0 != 0, explicit=True)
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(ga), _bits(gb))
    assert np.array_equal(metrics.masked_counts(_dev(t0)).cpu().numpy(), M.counts_brute(t0))
    assert np.array_equal(metrics.masked_counts(_dev(t0), _dev(v).bool()).cpu().numpy(), M.counts_brute(t0))     # a bool mask


@pytest.mark.parametrize("B,H,W", [(2, 40, 52), (1, 128, 128), (3, 9, 70)])
def test_all_valid_equals_the_unmasked_loss(B, H, W):
    from codon_amd.metrics import L1SSIMLoss
    p, t, _ = _case(B, H, W, seed=9)
    v = np.ones(p.shape, dtype=bool)
    lm, gm = _run(p, t, v, w=(1.0, 0.7))
    pd = _dev(p).requires_grad_(True)
    lu = L1SSIMLoss(1.0, 0.7)(pd, _dev(t))
    lu.backward()
    dl, rel = abs(float(lm) - float(lu.detach())), float((gm - pd.grad).double().norm() / pd.grad.double().norm())
    print(f"all-valid vs L1SSIMLoss {B}x{H}x{W}: |dloss| {dl:.3e} (bar 2e-6)  grad rel {rel:.3e} (bar 1e-6)")
    assert dl < 2e-6 and rel <= 1e-6


def test_shard_consistency():
    p, t, v = _case(4, 37, 53, seed=10, special=False)
    v[3, 0, :, :30] = False                                                     # very different valid counts per image
    lw, gw = _run(p, t, v)
    halves = [_run(p[s], t[s], v[s]) for s in (slice(0, 2), slice(2, 4))]
    mean = (float(halves[0][0].double()) + float(halves[1][0].double())) / 2
    gh = torch.cat([h[1] for h in halves]) / 2
    rel = float((gh - gw).double().norm() / gw.double().norm())
    print(f"shards: |mean of halves - batch| {abs(mean - float(lw)):.3e} (bar 1e-6)  grad rel {rel:.3e} (bar 2e-5)")
    assert abs(mean - float(lw)) <= 1e-6 and rel <= 2e-5
    for b in range(4):
        _, g1 = _run(p[b:b + 1], t[b:b + 1], v[b:b + 1])
        r = float((g1[0] / 4 - gw[b]).double().norm() / gw[b].double().norm())
        assert r <= 1e-6, (b, r)


def test_no_host_synchronisation():
    from codon_amd.metrics import MaskedL1SSIMLoss
    p, t, v = _case(5, 37, 53, seed=11)
    pd, td, vd = _dev(p).requires_grad_(True), _dev(np.where(v, t, 0.0)), _dev(v, torch.uint8)
    crit = MaskedL1SSIMLoss()
    crit(pd, td).backward()                                                     # library load, allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for valid in (None, vd):
            loss = crit(pd, td, valid)
            (loss * 0.5).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(pd.grad).all()


# ---- the label plane -----------------------------------------------------------------------------------------------------------

def _write_set(root, sizes, seed=0, label=True, smooth=False):
    """Depth maps without zeros, guidance, labels = ANOTHER image with holes (isolated zeros and a blob), so that a swap of
    the planes fails; `smooth`: something learnable, the label = the depth map with holes."""
    rng = np.random.default_rng(seed)
    dd, cd, ld = (os.path.join(root, n) for n in ("depth", "color", "label"))
    for d in (dd, cd, ld):
        os.makedirs(d, exist_ok=True)
    for i, (h, w) in enumerate(sizes):
        if smooth:
            yy, xx = np.mgrid[0:h, 0:w]
            d = (127.5 + 100 * np.sin(0.11 * yy + 0.3 * i) * np.cos(0.07 * xx)).astype(np.uint8).clip(1, 255)
            lab = d.copy()
        else:
            d = rng.integers(1, 256, size=(h, w), dtype=np.uint8)
            lab = rng.integers(1, 256, size=(h, w), dtype=np.uint8)
            lab.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
        lab[rng.random((h, w)) < 0.03] = 0
        if smooth:
            lab[:int(0.6 * h), :int(0.6 * w)] = 0                 # crops in the upper left fall under min_valid = 0.5
        else:
            lab[h // 3:h // 3 + 9, w // 4:w // 4 + 14] = 0
        g = np.clip(d.astype(int) + rng.integers(-20, 21, size=(h, w)), 0, 255).astype(np.uint8)
        io.write_gray(os.path.join(dd, f"{i:02d}.png"), d)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), np.pad(g, ((0, i % 3), (0, 1)), mode="edge"))
        if label:
            io.write_gray(os.path.join(ld, f"{i:02d}.png"), lab)
    return dd, cd, ld


@pytest.mark.parametrize("scale", [4, 8, 16])
def test_labeled_synthesis_bit_identical_to_numpy(tmp_path, scale):
    from tests import train_data_labeled_ref as RL
    from tests import train_data_ref as R
    P = 64
    dd, cd, ld = _write_set(str(tmp_path), [(70, 67), (64, 91), (97, 64)], seed=scale)
    ts = train.TrainSet(dd, cd, "cuda:0", crop=P, label_dir=ld)
    rows = []
    for op in range(8):                                          # every D4 code, the crop on every border
        i = op % 3
        off, (h, w) = int(ts.offsets[i]), ts.sizes[i].tolist()
        y0, x0 = [(0, 0), (h - P, w - P), (0, w - P), (h - P, 0)][op % 4]
        rows.append([off, h, w, y0, x0, op])
    descs = np.asarray(rows, dtype=np.int64)
    x, y, t = train.synthesize(ts, descs, scale, P)
    pool = ts.pool.cpu().numpy()
    rx, ry, rt = RL.synthesize(pool, descs, scale, P)
    for got, ref, n in ((t, rt, "t"), (y, ry, "y"), (x, rx, "x")):
        g = got.cpu().numpy()
        assert g.shape == ref.shape == (8, 1, P, P) and g.dtype == np.float32
        bad = np.argwhere(g.view(np.uint32) != ref.view(np.uint32))
        assert bad.size == 0, f"{n} x{scale}: {len(bad)} values differ, first at {bad[:3].tolist()}"
    # t is the label plane, x the degraded DEPTH plane: restated plane by plane, so that a swap fails
    for b, (off, h, w, y0, x0, op) in enumerate(rows):
        planes = [pool[off + k * h * w:off + (k + 1) * h * w].reshape(h, w) for k in range(3)]
        assert np.array_equal(t[b, 0].cpu().numpy(), R.lut()[R.d4(planes[2][y0:y0 + P, x0:x0 + P], op)])
        assert not np.array_equal(planes[0], planes[2])
    from oracle import upsample_oracle
    src = np.stack([R.lut()[R.d4(pool[o:o + h * w].reshape(h, w)[a:a + P, c:c + P], op)] for o, h, w, a, c, op in rows])[:, None]
    assert np.array_equal(x.cpu().numpy(), R.quantize(upsample_oracle.bicubic_upsample(R.downsample(src, scale), scale)))
    assert (t == 0).any() and not (x == 0).all()
    assert len(np.unique(t.cpu().numpy())) == 256


def test_unlabeled_set_takes_the_existing_entry(tmp_path):
    """Without a label directory synthesize is the existing path: the bits of tests/train_data_ref.py."""
    from tests import train_data_ref as R
    dd, cd, _ = _write_set(str(tmp_path), [(70, 67)], label=False)
    ts = train.TrainSet(dd, cd, "cuda:0", crop=64)
    descs = np.asarray([[0, 70, 67, 3, 2, 5]], dtype=np.int64)
    x, y, t = train.synthesize(ts, descs, 4, 64)
    rx, ry, rt = R.synthesize(ts.pool.cpu().numpy(), descs, 4, 64)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in ((x, rx), (y, ry), (t, rt)))


# ---- fit -----------------------------------------------------------------------------------------------------------------------

def _cli(dd, cd, ld, *extra):
    return ["--scale", "4", "--train-depth", dd, "--train-color", cd, "--train-label", ld, "--mask-holes", "--min-valid", "0.5",
            "--crop", "32", "--batch", "2", "--log-every", "1", "--seed", "5", *extra]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_masked_fit_resumes_bit_identically(tmp_path, dtype):
    dd, cd, ld = _write_set(str(tmp_path), [(48, 40), (40, 52), (44, 44)], smooth=True)
    a, b, c = (str(tmp_path / n) for n in ("a.pth", "b.pth", "c.pth"))
    lines = []
    straight = train.main(_cli(dd, cd, ld, "--dtype", dtype, "--steps", "4", "--save", a), emit=lines.append)
    train.main(_cli(dd, cd, ld, "--dtype", dtype, "--steps", "2", "--save", b), emit=lambda s: None)
    resumed = train.main(_cli(dd, cd, ld, "--dtype", dtype, "--steps", "4", "--resume", b, "--save", c), emit=lambda s: None)
    assert [s for s, _ in resumed["losses"]] == [3, 4] and resumed["losses"] == straight["losses"][2:]
    ca, cc = torch.load(a, weights_only=False), torch.load(c, weights_only=False)
    assert ca["epoch"] == cc["epoch"] == 4 and ca["rng"] == cc["rng"]
    for k, v in ca["model"].items():
        assert torch.equal(v, cc["model"][k]), k
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(ca["optimizer"][k], cc["optimizer"][k]), k
    assert ca["optimizer"]["t"] == cc["optimizer"]["t"] == 4
    for p, q in zip(straight["gs"].params, resumed["gs"].params):
        assert torch.equal(p, q)
    assert (ca["args"]["mask_holes"], ca["args"]["min_valid"], ca["args"]["train_label"]) == (True, 0.5, True)
    steps = [ln for ln in lines if ln.startswith("step ")]
    assert len(steps) == 4 and all(" valid 0." in ln or " valid 1.000" in ln for ln in steps), steps
    with pytest.raises(ValueError, match="mask_holes True != False"):           # the same data without the option: refused
        train.main(["--scale", "4", "--train-depth", dd, "--train-color", cd, "--crop", "32", "--batch", "2", "--resume", b])


def test_masked_fit_step_one_loss_and_valid_fraction(tmp_path):
    from codon_amd import CODONNet
    dd, cd, ld = _write_set(str(tmp_path), [(48, 40), (40, 52), (44, 44)], smooth=True)
    ts = train.TrainSet(dd, cd, "cuda:0", crop=32, label_dir=ld)
    torch.manual_seed(0)
    m = CODONNet().cuda()
    seen, lines = [], []
    h = m.register_forward_hook(lambda mod, inp, out: seen.append(out.detach().float().clone()))
    r = train.fit(m, ts, 1, scale=4, crop=32, batch=4, dtype="f32", seed=9, log_every=1, emit=lines.append, mask_holes=True,
                  min_valid=0.5)
    h.remove()
    descs = train.draw(np.random.default_rng(9), ts, 4, 32, min_valid=0.5)      # the rows fit drew
    _, _, t = train.synthesize(ts, descs, 4, 32)
    assert len(seen) == 1 and (t == 0).any()
    ref = float(M.masked_loss(seen[0].double().cpu(), t.double().cpu()))
    got = r["losses"][0][1]
    print(f"step-1 loss {got:.8f}, float64 restatement on the step's own output {ref:.8f}, |d| {abs(got - ref):.3e} (bar 2e-6)")
    assert abs(got - ref) < 2e-6
    frac = float((t != 0).double().mean())
    assert f" valid {frac:.3f}" in lines[0], (lines, frac)
    assert all((t[b] != 0).sum() >= 0.5 * 32 * 32 for b in range(4))
    with pytest.raises(ValueError, match="needs mask_holes"):
        train.fit(m, ts, 1, scale=4, crop=32, batch=4, min_valid=0.5, emit=lambda s: None)


def test_defaults_issue_the_same_calls(tmp_path):
    """With no new option a training step calls what it always called -- none of the new entries, one codon_train_crops,
    codon_ssim_fwd, codon_l1_fwd and codon_ssim_l1_bwd -- and the options change those calls ONLY: the rest of the ordered
    ABI log of the same step is identical."""
    from codon_amd import CODONNet
    from codon_amd import _lib as L
    spec = importlib.util.spec_from_file_location("abi_call_log", os.path.join(ROOT, "tools", "abi_call_log.py"))
    acl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(acl)
    dd, cd, ld = _write_set(str(tmp_path), [(48, 40), (40, 52)], smooth=True)
    new = {"codon_train_crops_labeled", "codon_masked_l1_ssim_fwd", "codon_masked_l1_ssim_bwd"}
    old = {"codon_train_crops", "codon_ssim_fwd", "codon_l1_fwd", "codon_ssim_l1_bwd"}
    real = L.load()
    logs = {}
    ts = train.TrainSet(dd, cd, "cuda:0", crop=32)
    train.fit(CODONNet().cuda(), ts, 1, scale=4, crop=32, batch=2, dtype="bf16", emit=lambda s: None)     # once-per-process work
    try:
        for key, label, kw in (("off", None, {}), ("on", ld, {"mask_holes": True, "min_valid": 0.25})):
            ts = train.TrainSet(dd, cd, "cuda:0", crop=32, label_dir=label)
            torch.manual_seed(0)
            m = CODONNet().cuda()
            fixed = np.asarray([[0, 48, 40, 2, 3, 1], [int(ts.offsets[1]), 40, 52, 5, 7, 6]], dtype=np.int64)
            log = acl.install()
            train.fit(m, ts, 2, scale=4, crop=32, batch=2, dtype="bf16", fixed=fixed, log_every=1, emit=lambda s: None, **kw)
            logs[key] = [(n, a) for n, a, _ in log]
            L._lib = real
    finally:
        L._lib = real
    names = {k: [n for n, _ in v] for k, v in logs.items()}
    assert not new & set(names["off"]) and all(names["off"].count(n) == 2 for n in old)
    assert not old & set(names["on"]) and all(names["on"].count(n) == 2 for n in new)
    rest = {k: [c for c in v if c[0] not in new | old] for k, v in logs.items()}
    assert rest["off"] == rest["on"] and len(rest["off"]) > 100
    swap = {"codon_train_crops": "codon_train_crops_labeled", "codon_ssim_fwd": "codon_masked_l1_ssim_fwd",
            "codon_ssim_l1_bwd": "codon_masked_l1_ssim_bwd"}
    assert [swap.get(n, n) for n in names["off"] if n != "codon_l1_fwd"] == names["on"]          # one launch pair less, same places
