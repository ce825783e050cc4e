"""codon_amd.train on the MI355X: the device-side batch synthesis is bit-identical to its numpy definition
(tests/train_data_ref.py), a repeated batch is fitted, --resume continues a run bit for bit, a checkpoint feeds
`python -m codon_amd.infer --weights`, and two ranks compute the one-process step.  Datasets are small synthetic PNGs."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from codon_amd import io, train

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_set(root, sizes, seed=0, color_extra=True):
    rng = np.random.default_rng(seed)
    dd, cd = os.path.join(root, "depth"), os.path.join(root, "color")
    os.makedirs(dd, exist_ok=True)
    os.makedirs(cd, exist_ok=True)
    for i, (h, w) in enumerate(sizes):
        # smooth depth (something to learn) with every u8 code present somewhere; noisy guidance
        yy, xx = np.mgrid[0:h, 0:w]
        d = (127.5 + 100 * np.sin(0.11 * yy + 0.3 * i) * np.cos(0.07 * xx)).astype(np.uint8)
        d.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
        g = np.clip(d.astype(int) + rng.integers(-20, 21, size=(h, w)), 0, 255).astype(np.uint8)
        if color_extra:                                          # guidance larger than the depth map: cropped to the common size
            g = np.pad(g, ((0, i % 3), (0, 1)), mode="edge")
        io.write_gray(os.path.join(dd, f"{i:02d}.png"), d)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), g)
    return dd, cd


@pytest.mark.parametrize("scale", [4, 8, 16])
def test_synthesize_bit_identical_to_numpy(tmp_path, scale):
    from tests import train_data_ref as R
    P = 64
    dd, cd = _write_set(str(tmp_path), [(70, 67), (64, 91), (97, 64)], seed=scale)
    ts = train.TrainSet(dd, cd, "cuda:0", crop=P)
    rows = []
    for op in range(8):                                          # every D4 code, the crop on every border
        i = op % 3
        off, (h, w) = int(ts.offsets[i]), ts.sizes[i].tolist()
        y0, x0 = [(0, 0), (h - P, w - P), (0, w - P), (h - P, 0)][op % 4]
        rows.append([off, h, w, y0, x0, op])
    descs = np.asarray(rows, dtype=np.int64)
    x, y, t = train.synthesize(ts, descs, scale, P)
    rx, ry, rt = R.synthesize(ts.pool.cpu().numpy(), descs, scale, P)
    for got, ref, n in ((t, rt, "t"), (y, ry, "y"), (x, rx, "x")):
        g = got.cpu().numpy()
        assert g.shape == ref.shape == (8, 1, P, P) and g.dtype == np.float32
        bad = np.argwhere(g.view(np.uint32) != ref.view(np.uint32))
        assert bad.size == 0, f"{n} x{scale}: {len(bad)} values differ, first at {bad[:3].tolist()}"
    assert len(np.unique(t.cpu().numpy())) == 256                       # every code went through the table
    assert not np.array_equal(rx, rt)                                   # the degradation did something


def test_synthesize_refusals(tmp_path):
    dd, cd = _write_set(str(tmp_path), [(40, 40)])
    ts = train.TrainSet(dd, cd, "cuda:0")
    with pytest.raises(ValueError, match="samples per launch"):
        train.synthesize(ts, np.zeros((65, 6), dtype=np.int64) + [0, 40, 40, 0, 0, 0], 4, 32)
    with pytest.raises(RuntimeError, match="outside the image"):
        train.synthesize(ts, np.asarray([[0, 40, 40, 9, 0, 0]]), 4, 32)
    with pytest.raises(RuntimeError, match="past the"):
        train.synthesize(ts, np.asarray([[1, 40, 40, 0, 0, 0]]), 4, 32)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_fixed_batch_overfit(tmp_path, dtype):
    from codon_amd import CODONNet
    dd, cd = _write_set(str(tmp_path), [(48, 40), (40, 52)])
    ts = train.TrainSet(dd, cd, "cuda:0", crop=32)
    fixed = train.draw(np.random.default_rng(1), ts, 2, 32)
    torch.manual_seed(0)
    m = CODONNet().cuda()
    r = train.fit(m, ts, 30, scale=4, crop=32, batch=2, lr=2e-4, dtype=dtype, fixed=fixed, log_every=1, emit=lambda s: None)
    losses = [v for _, v in r["losses"]]
    assert len(losses) == 30 and all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses


def _cli(dd, cd, *extra):
    return ["--scale", "4", "--train-depth", dd, "--train-color", cd, "--crop", "32", "--batch", "2", "--log-every", "1",
            "--seed", "5", *extra]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_resume_is_bit_identical_and_checkpoint_feeds_infer(tmp_path, dtype):
    from codon_amd import CODONNet, infer, metrics
    dd, cd = _write_set(str(tmp_path), [(48, 40), (40, 52), (44, 44)])
    a, b, c = (str(tmp_path / n) for n in ("a.pth", "b.pth", "c.pth"))
    quiet = lambda s: None                                               # noqa: E731
    straight = train.main(_cli(dd, cd, "--dtype", dtype, "--steps", "4", "--save", a), emit=quiet)
    train.main(_cli(dd, cd, "--dtype", dtype, "--steps", "2", "--save", b), emit=quiet)
    resumed = train.main(_cli(dd, cd, "--dtype", dtype, "--steps", "4", "--resume", b, "--save", c), emit=quiet)
    assert [s for s, _ in resumed["losses"]] == [3, 4]
    assert resumed["losses"] == straight["losses"][2:]
    ca, cc = torch.load(a, weights_only=False), torch.load(c, weights_only=False)
    assert ca["epoch"] == cc["epoch"] == 4 and ca["rng"] == cc["rng"]
    for k, v in ca["model"].items():
        assert torch.equal(v, cc["model"][k]), k
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(ca["optimizer"][k], cc["optimizer"][k]), k
    assert ca["optimizer"]["t"] == cc["optimizer"]["t"] == 4
    for p, q in zip(straight["gs"].params, resumed["gs"].params):
        assert torch.equal(p, q)

    # a refused optimizer state: the flat length must be the GradSync's
    bad = dict(ca["optimizer"], exp_avg=ca["optimizer"]["exp_avg"][:-1])
    with pytest.raises(ValueError, match="the GradSync holds"):
        resumed["opt"].load_state_dict(bad)
    if dtype != "f32":
        return

    # the checkpoint through io.load_checkpoint and `python -m codon_amd.infer --weights`
    fresh = CODONNet()
    assert io.load_checkpoint(a, fresh) == 4
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, ca["model"][k]), k
    out_dir = str(tmp_path / "out")
    assert infer.main(["--weights", a, "--dtype", "f32", "--out", out_dir, "--input-depth", dd, "--input-color", cd]) == 0
    m = straight["model"].eval()
    m.set_compute_dtype(None)
    for f in infer.list_pairs(dd, cd):
        px, py = io.read_gray(os.path.join(dd, f)), io.read_gray(os.path.join(cd, f))
        h, w = min(px.shape[0], py.shape[0]), min(px.shape[1], py.shape[1])
        with torch.no_grad():
            out = m(io.to_input(px[:h, :w]).cuda(), io.to_input(py[:h, :w]).cuda())
        want = metrics.postprocess_u8(out[0, 0]).cpu().numpy()
        assert np.array_equal(io.read_gray(os.path.join(out_dir, f)), want), f


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rel_worst(a, b, params):
    w, off = 0.0, 0
    for p in params:
        n = p.numel()
        x, y = a[off:off + n].double(), b[off:off + n].double()
        w = max(w, float((x - y).norm() / (y.norm() + 1e-30)))
        off += n
    return w


def _worker(rank, world, port, dd, cd, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.set_num_threads(2)
        torch.cuda.set_device(0)
        from codon_amd import CODONNet
        from codon_amd import train as T
        ts = T.TrainSet(dd, cd, "cuda:0", crop=32)
        solo = dist.new_group([0])
        res = {}
        for dtype in ("f32", "bf16"):
            torch.manual_seed(100 + rank)                     # different on each rank: the broadcast makes them equal
            m = CODONNet().cuda()
            r = T.fit(m, ts, 1, scale=4, crop=32, batch=4, dtype=dtype, seed=9, log_every=1, emit=lambda s: None)
            shard_loss, shard_grad = r["losses"][0][1], r["gs"].flat.clone()
            if rank == 0:
                torch.manual_seed(100)
                m1 = CODONNet().cuda()
                r1 = T.fit(m1, ts, 1, scale=4, crop=32, batch=4, dtype=dtype, seed=9, log_every=1, process_group=solo,
                           emit=lambda s: None)
                assert r1["world"] == 1 and r["world"] == 2
                res[dtype] = {"loss": (shard_loss, r1["losses"][0][1]),
                              "grad_rel": _rel_worst(shard_grad, r1["gs"].flat, r1["gs"].params)}
            dist.barrier()
        if rank == 0:
            q.put(("ok", res))
        dist.destroy_process_group()
    except BaseException as e:          # noqa: BLE001
        import traceback
        q.put(("err", f"rank {rank}: {e!r}\n{traceback.format_exc()}"))


def test_two_ranks_equal_one_process(tmp_path):
    dd, cd = _write_set(str(tmp_path), [(48, 40), (40, 52), (44, 44)])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, dd, cd, q)) for r in range(2)]
    for p in ps:
        p.start()
    try:
        kind, res = q.get(timeout=240)
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert kind == "ok", res
    for dtype, r in res.items():
        a, b = r["loss"]
        assert abs(a - b) <= 1e-6, (dtype, a, b)
        assert r["grad_rel"] <= 2e-5, (dtype, r["grad_rel"])
    assert all(p.exitcode == 0 for p in ps)
