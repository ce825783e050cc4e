"""Training on real low-resolution depth maps on the MI355X: codon_train_crops_lr is bit-identical to its numpy
restatement (tests/train_lr_ref.py), its x is the window and op of what inference builds from the whole file, synthesize makes
one launch and no synchronisation, a repeated batch is fitted, --resume continues a run bit for bit and the checkpoint feeds
`python -m codon_amd.infer --lr-depth`.  Small synthetic PNGs throughout."""
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, train
from tests import train_lr_ref as T

pytestmark = pytest.mark.gpu

SYNTH = ("codon_train_crops", "codon_train_crops_labeled", "codon_train_crops_u16", "codon_bicubic_downsample",
         "codon_bicubic_downsample_masked", "codon_bicubic_upsample", "codon_bicubic_upsample_masked", "codon_quantize_u8",
         "codon_quantize_levels")
CODES = [(8, 255), (16, 65535), (16, 4096)]


def _set(root, recs, s, bits, levels):
    dd, cd, ld = T.write_set(str(root), recs, bits)
    ts = train.TrainSet(dd, cd, "cuda:0", depth_bits=bits, depth_max=levels if bits == 16 else 65535, lr_dir=ld, scale=s)
    return ts, (dd, cd, ld)


def _check(ts, rows, s, bits, levels, what, min_share=None):
    """synthesize on the device against the restatement on the pool's own bytes: equal bits for x, y and t."""
    P = T.CROPS[s]
    descs = T.descs_of(rows, ts.offsets.tolist())
    x, y, t = train.synthesize(ts, descs, s, P)
    rx, ry, rt, branch = T.synthesize(ts.pool.cpu().numpy(), descs, s, P, bits, levels, with_branch=True)
    share = np.bincount(branch.reshape(-1), minlength=3) / branch.size
    print(f"{what}: {len(rows)} crops of {P}, branch shares [0 invalid, N/D, hole] = {np.round(100 * share, 1)} %")
    if min_share is not None:
        assert (share >= min_share).all(), share
    for got, ref, n in ((t, rt, "t"), (y, ry, "y"), (x, rx, "x")):
        g = got.cpu().numpy()
        assert g.shape == ref.shape == (len(rows), 1, P, P) and g.dtype == np.float32
        bad = np.argwhere(g.view(np.uint32) != ref.view(np.uint32))
        assert bad.size == 0, f"{what} {n}: {len(bad)} values differ, first at {bad[:3].tolist()}"
    return x, share


@pytest.mark.parametrize("bits,levels", CODES)
@pytest.mark.parametrize("s", [4, 8, 16])
def test_bit_identical_to_the_restatement(tmp_path, s, bits, levels):
    """Three 9 x 13 LR planes with the holes of "pattern", five windows each (the corners and an unaligned interior one), the
    eight D4 ops cycling; the restatement puts at least 10 % of the outputs in each branch of the rule."""
    recs, rows = T.case(s, levels)
    ts, _ = _set(tmp_path, recs, s, bits, levels)
    assert np.array_equal(ts.pool.cpu().numpy(), T.pack(recs, bits)[0])
    assert [r[3:5] for r in rows[10:15]] == [list(w) for w in T.windows(9 * s, 13 * s, T.CROPS[s])]
    y0, x0 = rows[14][3:5]
    assert y0 % s and x0 % s                                        # the interior window is aligned to no scale
    x, _ = _check(ts, rows, s, bits, levels, f"x{s} {bits}-bit /{levels}", min_share=0.10)
    assert (x == 0).any() and (x != 0).any()


@pytest.mark.parametrize("kind", ["none", "rowcol", "borders", "all", "one"])
def test_hole_kinds(tmp_path, kind):
    for s, bits, levels in ((4, 8, 255), (16, 16, 4096)):
        recs, rows = T.case(s, levels, kind=kind)
        ts, _ = _set(tmp_path / f"x{s}", recs, s, bits, levels)
        x, share = _check(ts, rows, s, bits, levels, f"{kind} x{s} {bits}-bit")
        if kind == "none":                                           # (an x of 0.0 is still possible: the cubic undershoots)
            assert share[0] == 1
        if kind == "all":
            assert share[2] == 1 and not x.any() and not torch.signbit(x).any()


@pytest.mark.parametrize("bits,levels", [(8, 255), (16, 4096)])
def test_mixed_sizes_and_batch_extremes(tmp_path, bits, levels):
    s = 4
    recs, rows = T.case(s, levels, shapes=((9, 13), (5, 7)))
    ts, _ = _set(tmp_path, recs, s, bits, levels)
    assert ts.sizes.tolist() == [[36, 52], [20, 28]]
    _check(ts, rows, s, bits, levels, "mixed sizes")                 # ten windows of both images in one batch
    _check(ts, rows[9:10], s, bits, levels, "B = 1")                 # the unaligned interior window of the small image
    many = [rows[k % len(rows)][:5] + [(k + k // 8) % 8] for k in range(L.TRAIN_MAX_BATCH)]
    _check(ts, many, s, bits, levels, "B = 64")


def _d4(c, op):
    if op & 1:
        c = c.T
    if op & 2:
        c = c.flip(0)
    if op & 4:
        c = c.flip(1)
    return c


@pytest.mark.parametrize("bits,levels", [(8, 255), (16, 4096)])
@pytest.mark.parametrize("s", [4, 16])
def test_x_is_the_window_of_inferences_input(tmp_path, s, bits, levels):
    """Both sides on the GPU: synthesize's x against the window and op of infer.codes_to_input(whole LR codes, fp32)."""
    recs, rows = T.case(s, levels)
    ts, _ = _set(tmp_path, recs, s, bits, levels)
    P = T.CROPS[s]
    x, _, _ = train.synthesize(ts, T.descs_of(rows, ts.offsets.tolist()), s, P)
    whole = []
    for _, _, lr in recs:
        codes = torch.from_numpy(lr.view(np.int16) if bits == 16 else lr).cuda()
        whole.append(infer.codes_to_input(codes, s, torch.float32, levels if bits == 16 else None)[0, 0])
    for b, (i, H, W, y0, x0, op) in enumerate(rows):
        assert whole[i].shape == (H, W)
        assert torch.equal(x[b, 0], _d4(whole[i][y0:y0 + P, x0:x0 + P], op)), (b, i, y0, x0, op)


@pytest.mark.parametrize("bits,levels", [(8, 255), (16, 4096)])
def test_one_launch_and_no_synchronisation(tmp_path, bits, levels):
    from tests.abi_log_8bit import _acl
    s, P = 8, T.CROPS[8]
    recs, rows = T.case(s, levels)
    ts, _ = _set(tmp_path, recs, s, bits, levels)
    descs = T.descs_of(rows, ts.offsets.tolist())
    want = train.synthesize(ts, descs, s, P)                        # the tables go up on first use
    torch.cuda.synchronize()
    real = L.load()
    log = _acl().install()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = train.synthesize(ts, descs, s, P)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        L._lib = real
    names = [n for n, _, _ in log]
    assert names == ["codon_train_crops_lr"], names
    assert not set(names) & set(SYNTH)
    args = log[0][1]
    assert args[0]["n"] == len(rows) and args[0]["crop"] == P and args[3:5] == [s, bits] and args[6] == levels and log[0][2] == 0
    for g, w in zip(got, want):
        assert g.shape == (len(rows), 1, P, P) and g.dtype == torch.float32 and torch.equal(g, w)


# ---- training --------------------------------------------------------------------------------------------------------------------

def _write_pairs(root, sizes, s=4, seed=0):
    """HR depth as smooth as tests/test_gpu_train.py's, its guidance, and LR files that sample the depth map at
    [s//2::s, s//2::s] with about 6 % of the codes set to 0."""
    rng = np.random.default_rng(seed)
    dd, cd, ld = (os.path.join(root, n) for n in ("depth", "color", "lr"))
    for d in (dd, cd, ld):
        os.makedirs(d, exist_ok=True)
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        d = (127.5 + 100 * np.sin(0.11 * yy + 0.3 * i) * np.cos(0.07 * xx)).astype(np.uint8)
        g = np.clip(d.astype(int) + rng.integers(-20, 21, size=(h, w)), 0, 255).astype(np.uint8)
        g = np.pad(g, ((0, i % 3), (0, 1)), mode="edge")           # guidance larger than the depth map: cropped
        lr = d[s // 2::s, s // 2::s].copy()
        lr[rng.uniform(size=lr.shape) < 0.06] = 0
        io.write_gray(os.path.join(dd, f"{i:02d}.png"), d)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), g)
        io.write_gray(os.path.join(ld, f"{i:02d}.png"), lr)
    return dd, cd, ld


def test_fixed_batch_overfit(tmp_path):
    from codon_amd import CODONNet
    dd, cd, ld = _write_pairs(str(tmp_path), [(48, 40), (40, 52)])
    ts = train.TrainSet(dd, cd, "cuda:0", crop=32, lr_dir=ld, scale=4)
    fixed = train.draw(np.random.default_rng(1), ts, 2, 32)
    torch.manual_seed(0)
    m = CODONNet().cuda()
    r = train.fit(m, ts, 30, scale=4, crop=32, batch=2, lr=2e-4, dtype="bf16", fixed=fixed, log_every=1, emit=lambda s: None)
    losses = [v for _, v in r["losses"]]
    print(f"losses: first {losses[0]:.6f}, last {losses[-1]:.6f}")
    assert len(losses) == 30 and all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses


def test_cli_resume_validation_and_infer(tmp_path):
    dd, cd, ld = _write_pairs(str(tmp_path), [(48, 40), (40, 52), (44, 44)])
    a, b, c = (str(tmp_path / n) for n in ("a.pth", "b.pth", "c.pth"))
    quiet = lambda s: None                                               # noqa: E731

    def cli(*extra):
        return ["--scale", "4", "--train-depth", dd, "--train-color", cd, "--train-lr-depth", ld, "--mask-holes", "--crop", "32",
                "--batch", "2", "--log-every", "1", "--seed", "5", "--dtype", "bf16", *extra]

    lines = []
    straight = train.main(cli("--steps", "4", "--save", a, "--val-lr-depth", ld, "--val-color", cd, "--val-label", dd,
                              "--val-every", "4"), emit=lines.append)
    val = [ln for ln in lines if ln.startswith("val ")]
    assert len(val) == 1 and val[0].startswith("val 3 images rmse ") and " ssim " in val[0], lines
    train.main(cli("--steps", "2", "--save", b), emit=quiet)
    resumed = train.main(cli("--steps", "4", "--resume", b, "--save", c), emit=quiet)
    assert [s for s, _ in resumed["losses"]] == [3, 4]
    assert resumed["losses"] == straight["losses"][2:]
    ca, cc = torch.load(a, weights_only=False), torch.load(c, weights_only=False)
    assert ca["epoch"] == cc["epoch"] == 4 and ca["rng"] == cc["rng"]
    assert ca["args"]["train_lr_depth"] is True and cc["args"]["train_lr_depth"] is True and ca["args"]["mask_holes"] is True
    for k, v in ca["model"].items():
        assert torch.equal(v, cc["model"][k]), k
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(ca["optimizer"][k], cc["optimizer"][k]), k
    assert ca["optimizer"]["t"] == cc["optimizer"]["t"] == 4
    for p, q in zip(straight["gs"].params, resumed["gs"].params):
        assert torch.equal(p, q)
    # the key is compared on --resume, before any GPU work: a run without the option refuses this checkpoint
    with pytest.raises(ValueError, match="train_lr_depth True != False"):
        train.main([v for v in cli("--steps", "4", "--resume", b) if v not in ("--train-lr-depth", ld)], emit=quiet)

    # the checkpoint in `python -m codon_amd.infer --lr-depth`: the forward of the trained model on codes_to_input's planes
    from codon_amd import metrics
    out_dir = str(tmp_path / "out")
    assert infer.main(["--scale", "4", "--weights", a, "--dtype", "f32", "--out", out_dir, "--lr-depth", ld, "--input-color", cd]) == 0
    m = straight["model"].eval()
    m.set_compute_dtype(None)
    for f in infer.list_pairs(ld, cd):
        lr, py = io.read_gray(os.path.join(ld, f)), io.read_gray(os.path.join(cd, f))
        h, w = lr.shape[0] * 4, lr.shape[1] * 4
        with torch.no_grad():
            out = m(infer.codes_to_input(torch.from_numpy(np.array(lr)).cuda(), 4, torch.float32), io.to_input(py[:h, :w]).cuda())
        assert np.array_equal(io.read_gray(os.path.join(out_dir, f)), metrics.postprocess_u8(out[0, 0]).cpu().numpy()), f
