"""The guarded training step on the MI355X (codon_grad_norm + codon_adam_step_guarded behind codon_amd.dist.FlatAdam's
max_norm / skip_nonfinite / ema_decay, and codon_amd.train's options on top): the norm against float64, nothing firing =
the plain step bit for bit, clipping + EMA against the update restated in float64 with the fp32 torch twin as the yardstick,
non-finite steps skipped whole, no hidden synchronisation, bit-identical resume, two ranks, EMA checkpoints."""
import ctypes as C
import functools
import hashlib
import os
import socket
import struct
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from codon_amd import io, train
from oracle import codon_oracle as orc
from tests.util import rel_rmse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _gs(seed=31):
    from codon_amd import CODONNet
    from codon_amd.dist import GradSync
    m = CODONNet()
    m.load_state_dict(orc.he_state("x4", seed=seed), strict=True)
    m = m.cuda().train()
    return m, GradSync(m)


def _flat(params):
    return torch.cat([p.detach().reshape(-1) for p in params])


def _bits(x: float) -> bytes:
    return struct.pack("<d", x)


# ---- kernel level ---------------------------------------------------------------------------------------------------------------

def test_norm_against_float64():
    """stats()["norm"] against the float64 norm of the same buffer to 1e-9 relative (float64 accumulation of exact products:
    n * 2^-53 = 2e-10 for the kernel, the same order for torch's float64 sum) at magnitudes 1e-20 .. 3e18 (fp32 squares would
    underflow / overflow at both ends); a single non-zero element and the all-zero buffer exactly; equal bits call to call.
    The flat length, 1 865 506 = 2 mod 4, exercises the scalar tail."""
    from codon_amd.dist import FlatAdam
    _, gs = _gs()
    assert gs.numel % 4 == 2
    opt = FlatAdam(gs, lr=1e-3, skip_nonfinite=True)
    g = torch.Generator(device="cpu").manual_seed(11)
    for s in (1e-20, 1e-4, 1.0, 3e18):
        gs.flat.copy_(torch.randn(gs.numel, generator=g) * s)
        opt.step()
        got, want = opt.stats()["norm"], float(gs.flat.double().norm())
        print(f"norm at scale {s:g}: kernel {got!r} float64 {want!r} rel {abs(got - want) / want:.3e}")
        assert abs(got - want) <= 1e-9 * want, s
        part = opt._state[4:].clone()
        opt.step()                                                        # the same buffer again: the same bits
        assert _bits(opt.stats()["norm"]) == _bits(got) and torch.equal(opt._state[4:], part)
    for x in (-1.2345678e-3, 3e18, 1e-20):                                # zero except the last element (the tail's last)
        gs.flat.zero_()
        gs.flat[-1] = x
        opt.step()
        assert opt.stats()["norm"] == abs(float(gs.flat[-1])), x
    assert opt.stats()["skipped"] == 0

    # the all-zero buffer: norm exactly 0, and the step it feeds is applied unclipped (= the plain step on a zero gradient)
    (_, gsa), (_, gsb) = _gs(), _gs()
    a, b = FlatAdam(gsa, lr=1e-3, weight_decay=1e-2, max_norm=1.0, skip_nonfinite=True), FlatAdam(gsb, lr=1e-3, weight_decay=1e-2)
    a.step()
    b.step()
    st = a.stats()
    assert _bits(st["norm"]) == _bits(0.0) and (st["applied"], st["skipped"], st["clipped"]) == (1, 0, 0)
    assert torch.equal(_flat(gsa.params), _flat(gsb.params)) and torch.equal(a.exp_avg, b.exp_avg)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_nothing_fires_nothing_changes(wd):
    """max_norm = inf and a finite gradient: the guarded step is codon_adam_step bit for bit (parameters, both moments), on
    the five gradients of test_flat_adam_equals_torch_optim_adam."""
    from codon_amd.dist import FlatAdam
    (_, gsa), (_, gsb) = _gs(), _gs()
    a = FlatAdam(gsa, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, max_norm=INF, skip_nonfinite=True)
    b = FlatAdam(gsb, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd)
    assert a.guarded and not b.guarded
    g = torch.Generator(device="cpu").manual_seed(5)
    v0 = [p._version for p in gsa.params]
    for step in range(5):
        grad = (torch.randn(gsa.numel, generator=g) * (0.5 + step)).cuda()
        gsa.flat.copy_(grad)
        gsb.flat.copy_(grad)
        a.step()
        b.step()
        assert torch.equal(gsa.flat, grad)                                # the gradient buffer is left as it was
    assert all(p._version > v for p, v in zip(gsa.params, v0))
    for (n, pa), pb in zip(gsa.named, gsb.params):
        assert torch.equal(pa, pb), n
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    st = a.stats()
    assert (st["applied"], st["skipped"], st["clipped"]) == (5, 0, 0)


HYPER = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8)
MAX_NORM_A, DECAY_A = 3000.0, 0.9     # the five norms are (0.5 + k) * sqrt(1 865 506) = 683, 2 049, 3 415, 4 781, 6 147


def _ref64(p0, grads, wd, max_norm, decay):
    """clip_grad_norm_ + torch.optim.Adam + the EMA recurrence in float64 on the CPU; returns (p, ema, steps clipped)."""
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([p], weight_decay=wd, **HYPER)
    ema, clipped = p.detach().clone(), 0
    for g in grads:
        p.grad = g.double().clone()
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm)
        clipped += int(max_norm / (float(norm) + 1e-6) < 1.0)
        opt.step()
        ema += (1.0 - decay) * (p.detach() - ema)
    return p.detach(), ema, clipped


@functools.lru_cache(maxsize=None)
def _sequence_a(wd):
    """Sequence A through the kernels, the fp32 torch twin and the float64 reference: {"yard": the twin's four rel_rmse to the
    reference (parameters, update, EMA, EMA's movement), "got": the kernels' four, "clipped": (kernels, reference)}."""
    from codon_amd.dist import FlatAdam
    (_, gsa), (_, gsb) = _gs(), _gs()
    p0 = _flat(gsa.params).cpu()
    a = FlatAdam(gsa, weight_decay=wd, max_norm=MAX_NORM_A, ema_decay=DECAY_A, **HYPER)
    b = torch.optim.Adam(gsb.params, weight_decay=wd, **HYPER)
    ema_b = [p.detach().clone() for p in gsb.params]
    gen = torch.Generator(device="cpu").manual_seed(5)
    grads = [torch.randn(gsa.numel, generator=gen) * (0.5 + k) for k in range(5)]
    for g in grads:
        gsa.flat.copy_(g)
        gsb.flat.copy_(g)
        a.step()
        torch.nn.utils.clip_grad_norm_(gsb.params, MAX_NORM_A)
        b.step()
        with torch.no_grad():
            torch._foreach_lerp_(ema_b, [p.detach() for p in gsb.params], 1.0 - DECAY_A)     # torch.optim.swa_utils' EMA form
    p64, e64, clipped64 = _ref64(p0, grads, wd, MAX_NORM_A, DECAY_A)
    p0 = p0.double()

    def four(p, e):
        p, e = p.cpu().double(), e.cpu().double()
        return (rel_rmse(p, p64), rel_rmse(p - p0, p64 - p0), rel_rmse(e, e64), rel_rmse(e - p0, e64 - p0))

    return {"yard": four(_flat(gsb.params), _flat(ema_b)), "got": four(_flat(gsa.params), a.ema),
            "clipped": (a.stats()["clipped"], clipped64), "applied": a.stats()["applied"]}


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_clipping_and_ema_against_float64(wd):
    """Five gradients with norms on both sides of max_norm, EMA decay 0.9.  Reference: the update in float64.  Bound: 2 x the
    fp32 torch twin's own rel_rmse to that reference, measured in this run, for the parameters, the update, the EMA and the
    EMA's movement (same fp32 arithmetic in another operation order; the float64 norm can only help)."""
    r = _sequence_a(wd)
    names = ("parameters", "update", "ema", "ema movement")
    for n, y, got in zip(names, r["yard"], r["got"]):
        print(f"wd {wd:g} {n}: fp32 torch twin {y:.3e} kernels {got:.3e} ratio {got / y:.3f}")
    assert r["clipped"][1] == 3 and r["clipped"][0] == r["clipped"][1] and r["applied"] == 5
    for n, y, got in zip(names, r["yard"], r["got"]):
        assert got <= 2 * y, (n, got, y)


def test_overflow_hole():
    """g = 3e18 * randn, max_norm = 1: the squares overflow fp32, so torch's fp32 clip_grad_norm_ sees norm = inf, scales the
    gradient by 0 and the step moves nothing -- which is why the reference of these tests is float64, not the fp32 twin.  The
    kernels' float64 norm clips the step instead: its update is held to sequence A's update bound against float64."""
    from codon_amd.dist import FlatAdam
    (_, gsa), (_, gsb) = _gs(), _gs()
    p0 = _flat(gsa.params).cpu()
    g = torch.randn(gsa.numel, generator=torch.Generator(device="cpu").manual_seed(7)) * 3e18
    a = FlatAdam(gsa, max_norm=1.0, skip_nonfinite=True, **HYPER)
    gsa.flat.copy_(g)
    a.step()
    st = a.stats()
    assert (st["applied"], st["skipped"], st["clipped"]) == (1, 0, 1) and np.isfinite(st["norm"])
    p64, _, clipped64 = _ref64(p0, [g], 0.0, 1.0, 0.0)
    got = rel_rmse(_flat(gsa.params).cpu().double() - p0.double(), p64 - p0.double())
    bound = 2 * _sequence_a(0.0)["yard"][1]
    print(f"overflow hole: update rel_rmse to float64 {got:.3e}, bound {bound:.3e}")
    assert clipped64 == 1 and got <= bound

    b = torch.optim.Adam(gsb.params, **HYPER)
    gsb.flat.copy_(g)
    norm = torch.nn.utils.clip_grad_norm_(gsb.params, 1.0)
    b.step()
    moved = float((_flat(gsb.params).cpu() - p0).abs().max())
    print(f"overflow hole: the fp32 torch twin sees norm {float(norm)} and moves the parameters by {moved} (a dropped step)")
    assert torch.isinf(norm) and moved == 0.0


def test_nonfinite_steps_are_skipped_whole():
    """NaN, +Inf, -Inf at the first element, the last element and inside a middle tensor: parameters, moments and EMA keep
    their bits, `skipped` goes up and `applied` does not; the next finite step is, bit for bit, the step of a twin that never
    saw the bad gradients but had its step count advanced by as many.  With skip_nonfinite=False nothing is hidden: a NaN norm
    gives a NaN coefficient (all parameters turn NaN), an Inf norm the coefficient 0 and 0 * Inf = NaN, so at least the poisoned
    element's parameter turns non-finite, as torch.optim.Adam's would behind clip_grad_norm_."""
    from codon_amd.dist import FlatAdam
    (_, gsa), (_, gsb) = _gs(), _gs()
    kw = dict(weight_decay=1e-2, max_norm=2000.0, skip_nonfinite=True, ema_decay=0.9, **HYPER)
    a, b = FlatAdam(gsa, **kw), FlatAdam(gsb, **kw)
    gen = torch.Generator(device="cpu").manual_seed(13)
    g0, g1 = (torch.randn(gsa.numel, generator=gen).cuda() for _ in range(2))
    for gs, o in ((gsa, a), (gsb, b)):
        gs.flat.copy_(g0)
        o.step()
    mid = sum(p.numel() for p in gsa.params[:20]) + gsa.params[20].numel() // 2
    snap = [t.clone() for t in (_flat(gsa.params), a.exp_avg, a.exp_avg_sq, a.ema)]
    n = 0
    for bad in (float("nan"), INF, -INF):
        for where in (0, gsa.numel - 1, mid):
            gsa.flat.copy_(g1)
            gsa.flat[where] = bad
            a.step()
            n += 1
            st = a.stats()
            assert (st["applied"], st["skipped"]) == (1, n), (bad, where, st)
            for was, now in zip(snap, (_flat(gsa.params), a.exp_avg, a.exp_avg_sq, a.ema)):
                assert torch.equal(was.view(torch.int32), now.view(torch.int32)), (bad, where)
    b.t += n                                          # a skipped step consumes its step number
    for gs, o in ((gsa, a), (gsb, b)):
        gs.flat.copy_(g1)
        o.step()
    assert a.t == b.t == n + 2 and a.stats()["applied"] == 2
    for x, y in zip((_flat(gsa.params), a.exp_avg, a.exp_avg_sq, a.ema), (_flat(gsb.params), b.exp_avg, b.exp_avg_sq, b.ema)):
        assert torch.equal(x, y)
    assert not torch.equal(_flat(gsa.params), snap[0])

    for bad in (float("nan"), INF, -INF):
        _, gsc = _gs()
        c = FlatAdam(gsc, max_norm=1.0, skip_nonfinite=False, **HYPER)
        gsc.flat.copy_(g1)
        gsc.flat[mid] = bad
        c.step()
        st = c.stats()
        assert (st["applied"], st["skipped"]) == (1, 0)
        assert not bool(torch.isfinite(_flat(gsc.params)[mid])), bad


def test_step_does_not_synchronise():
    from codon_amd.dist import FlatAdam
    _, gs = _gs()
    opt = FlatAdam(gs, max_norm=1.0, skip_nonfinite=True, ema_decay=0.99, **HYPER)
    gs.flat.copy_(torch.randn(gs.numel))
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(10):
            opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    st = opt.stats()
    assert (st["applied"], st["clipped"]) == (10, 10)


def test_guarded_step_refusals_on_the_gpu():
    from codon_amd import _lib as L
    from tests.test_train_guard_cpu import guarded_refusals
    buf = torch.zeros(4096, device="cuda")
    guarded_refusals(L.load(), C.c_void_p(buf.data_ptr()), L)
    torch.cuda.synchronize()
    assert not buf.any()                                                  # nothing was launched


def test_flat_adam_state_round_trip_and_refusals():
    from codon_amd.dist import FlatAdam
    (_, gsa), (_, gsb) = _gs(), _gs()
    for bad in (dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=float("nan")), dict(ema_decay=1.0), dict(ema_decay=-0.1)):
        with pytest.raises(ValueError, match="FlatAdam"):
            FlatAdam(gsa, **bad)
    a = FlatAdam(gsa, max_norm=500.0, skip_nonfinite=True, ema_decay=0.9, **HYPER)
    for k in range(3):
        gsa.flat.copy_(torch.randn(gsa.numel) * (0.2 + 0.2 * k))
        if k == 1:
            gsa.flat[5] = INF
        a.step(lr=1e-3 * (k + 1))
    sd = a.state_dict()
    assert (sd["applied"], sd["skipped"], sd["clipped"], sd["lr"]) == (2, 1, 1, 3e-3)
    b = FlatAdam(gsb, lr=1.0)
    b.load_state_dict(sd)
    assert b.guarded and (b.max_norm, b.skip_nonfinite, b.ema_decay, b.t, b.lr) == (500.0, True, 0.9, 3, 3e-3)
    assert torch.equal(b.ema, a.ema)
    assert {k: v for k, v in b.stats().items() if k != "norm"} == {k: v for k, v in a.stats().items() if k != "norm"}
    with pytest.raises(ValueError, match="the GradSync holds"):
        b.load_state_dict(dict(sd, ema=sd["ema"][:-1]))
    b.load_state_dict({k: sd[k] for k in ("exp_avg", "exp_avg_sq", "t", "lr", "betas", "eps", "weight_decay")})     # an old state
    assert not b.guarded and b.ema is None


# ---- through train.fit / the command line ------------------------------------------------------------------------------------------

def _write_set(root, sizes, seed=0, color_extra=True):
    rng = np.random.default_rng(seed)
    dd, cd = os.path.join(root, "depth"), os.path.join(root, "color")
    os.makedirs(dd, exist_ok=True)
    os.makedirs(cd, exist_ok=True)
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        d = (127.5 + 100 * np.sin(0.11 * yy + 0.3 * i) * np.cos(0.07 * xx)).astype(np.uint8)
        d.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
        g = np.clip(d.astype(int) + rng.integers(-20, 21, size=(h, w)), 0, 255).astype(np.uint8)
        if color_extra:
            g = np.pad(g, ((0, i % 3), (0, 1)), mode="edge")
        io.write_gray(os.path.join(dd, f"{i:02d}.png"), d)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), g)
    return dd, cd


def _cli(dd, cd, *extra):
    return ["--scale", "4", "--train-depth", dd, "--train-color", cd, "--crop", "32", "--batch", "2", "--log-every", "1",
            "--seed", "5", *extra]


quiet = lambda s: None                                                       # noqa: E731


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_guarded_resume_is_bit_identical(tmp_path, dtype):
    dd, cd = _write_set(str(tmp_path), [(48, 40), (40, 52), (44, 44)])
    a, b, c = (str(tmp_path / n) for n in ("a.pth", "b.pth", "c.pth"))
    curve = ["--skip-nonfinite", "--ema", "0.9", "--lr-schedule", "cosine", "--lr-steps", "6", "--warmup-steps", "2", "--lr-min", "1e-6"]
    lines = []
    train.main(_cli(dd, cd, "--dtype", dtype, "--steps", "6", *curve), emit=lines.append)
    norms = [float(ln.split(" gnorm ")[1].split()[0]) for ln in lines if " gnorm " in ln]
    assert len(norms) == 6 and all(np.isfinite(norms)) and min(norms) < max(norms), lines
    clip = ["--clip-norm", repr(0.5 * (min(norms) + max(norms)))]             # between the smallest and the largest norm seen
    print(f"{dtype}: unclipped norms {norms}, {' '.join(clip)}")
    straight = train.main(_cli(dd, cd, "--dtype", dtype, "--steps", "6", "--save", a, *curve, *clip), emit=quiet)
    train.main(_cli(dd, cd, "--dtype", dtype, "--steps", "3", "--save", b, *curve, *clip), emit=quiet)
    resumed = train.main(_cli(dd, cd, "--dtype", dtype, "--steps", "6", "--resume", b, "--save", c, *curve, *clip), emit=quiet)
    st = straight["stats"]
    assert st["applied"] == 6 and st["skipped"] == 0 and 1 <= st["clipped"] <= 5, st
    assert resumed["stats"] == st
    assert [s for s, _ in resumed["losses"]] == [4, 5, 6] and resumed["losses"] == straight["losses"][3:]
    ca, cc = torch.load(a, weights_only=False), torch.load(c, weights_only=False)
    assert ca["epoch"] == cc["epoch"] == 6 and ca["rng"] == cc["rng"] and ca["args"] == cc["args"]
    for key in ("model", "model_ema"):
        for k, v in ca[key].items():
            assert torch.equal(v, cc[key][k]), (key, k)
    for k in ("exp_avg", "exp_avg_sq", "ema"):
        assert torch.equal(ca["optimizer"][k], cc["optimizer"][k]), k
    for k in ("t", "applied", "skipped", "clipped", "lr", "max_norm", "skip_nonfinite", "ema_decay"):
        assert ca["optimizer"][k] == cc["optimizer"][k], k
    assert ca["optimizer"]["lr"] == train.lr_at(6, lr=1e-4, schedule="cosine", warmup=2, lr_min=1e-6, lr_steps=6) == 1e-6
    for p, q in zip(straight["gs"].params, resumed["gs"].params):
        assert torch.equal(p, q)
    assert torch.equal(straight["opt"].ema, resumed["opt"].ema)

    # a cosine checkpoint under another curve length is another trajectory
    with pytest.raises(ValueError, match="other arguments.*lr_steps"):
        train.main(_cli(dd, cd, "--dtype", dtype, "--steps", "8", "--resume", b, *curve[:5], "--lr-steps", "8", *curve[7:], *clip), emit=quiet)


def test_grad_hook_poison_is_skipped(tmp_path):
    from codon_amd import CODONNet
    dd, cd = _write_set(str(tmp_path), [(48, 40), (40, 52)])
    ts = train.TrainSet(dd, cd, "cuda:0", crop=32)
    fixed = train.draw(np.random.default_rng(1), ts, 2, 32)

    def run(skip):
        seen = {}

        def hook(step, gs):
            seen[step] = _flat(gs.params).clone()                         # the parameters after step - 1
            if step == 3:
                gs.flat[12345] = INF

        torch.manual_seed(0)
        m = CODONNet().cuda()
        r = train.fit(m, ts, 5, scale=4, crop=32, batch=2, lr=2e-4, dtype="f32", fixed=fixed, log_every=1, emit=quiet,
                      skip_nonfinite=skip, grad_hook=hook)
        return r, seen

    r, seen = run(True)
    assert torch.equal(seen[4], seen[3]) and not torch.equal(seen[3], seen[2]) and not torch.equal(seen[5], seen[4])
    assert r["stats"]["skipped"] == 1 and r["stats"]["applied"] == 4
    losses = [v for _, v in r["losses"]]
    assert len(losses) == 5 and all(np.isfinite(losses)) and losses[4] < losses[0], losses
    r, _ = run(False)                                                     # the failure the option removes, shown once
    assert "stats" not in r
    assert not bool(torch.isfinite(_flat(r["gs"].params)).all())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


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

        def hook(step, gs):
            if step == 2 and rank == 1:                                   # one rank's shard alone: the all-reduce spreads it
                gs.flat[777] = float("inf")

        torch.manual_seed(100 + rank)
        m = CODONNet().cuda()
        r = T.fit(m, ts, 3, scale=4, crop=32, batch=4, dtype="bf16", seed=9, log_every=1, emit=lambda s: None,
                  skip_nonfinite=True, clip_norm=1e3, grad_hook=hook)
        flat = torch.cat([p.detach().reshape(-1) for p in r["gs"].params]).cpu()
        dist.barrier()
        q.put(("ok", rank, r["stats"], hashlib.sha256(flat.numpy().tobytes()).hexdigest(), bool(torch.isfinite(flat).all())))
        dist.destroy_process_group()
    except BaseException as e:          # noqa: BLE001
        import traceback
        q.put(("err", rank, f"rank {rank}: {e!r}\n{traceback.format_exc()}", None, None))


def test_two_ranks_skip_together(tmp_path):
    dd, cd = _write_set(str(tmp_path), [(48, 40), (40, 52), (44, 44)])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, dd, cd, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = []
    try:
        for _ in ps:
            got.append(q.get(timeout=240))
            if got[-1][0] != "ok":
                break
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(g[0] == "ok" for g in got) and len(got) == 2, got
    by_rank = {g[1]: g for g in got}
    for rank in (0, 1):
        assert by_rank[rank][2]["skipped"] == 1 and by_rank[rank][2]["applied"] == 2, by_rank[rank]
        assert by_rank[rank][4]
    assert by_rank[0][3] == by_rank[1][3]                                  # bit-identical parameters
    assert all(p.exitcode == 0 for p in ps)


def test_ema_checkpoint_and_old_checkpoints(tmp_path):
    from codon_amd import CODONNet, infer, metrics
    dd, cd = _write_set(str(tmp_path), [(48, 40), (40, 52), (44, 44)])
    e, plain, old = (str(tmp_path / n) for n in ("ema.pth", "plain.pth", "old.pth"))
    res = train.main(_cli(dd, cd, "--dtype", "f32", "--steps", "4", "--save", e, "--ema", "0.9", "--lr", "1e-3"), emit=quiet)
    ck = torch.load(e, weights_only=False)
    ref = CODONNet().state_dict()
    assert [(k, tuple(v.shape)) for k, v in ck["model_ema"].items()] == [(k, tuple(v.shape)) for k, v in ref.items()]
    used = {n for n, _ in res["gs"].named}
    assert len(used) == 44 and len(ref) == 49
    assert any(not torch.equal(ck["model_ema"][k], ck["model"][k]) for k in used)
    for k in ref:
        if k not in used:
            assert "attention_c5" in k or "attention_s5" in k, k
            assert torch.equal(ck["model_ema"][k], ck["model"][k]), k
    off = 0
    for n, p in res["gs"].named:                                          # the 44 used tensors are the optimizer's flat EMA
        assert torch.equal(ck["model_ema"][n].reshape(-1), ck["optimizer"]["ema"][off:off + p.numel()]), n
        off += p.numel()

    fresh = CODONNet()
    assert io.load_checkpoint(e, fresh, ema=True) == 4
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, ck["model_ema"][k]), k
    out_dir = str(tmp_path / "out")
    assert infer.main(["--weights", e, "--ema", "--dtype", "f32", "--out", out_dir, "--input-depth", dd, "--input-color", cd]) == 0
    m = fresh.cuda().eval()
    for f in infer.list_pairs(dd, cd):
        px, py = io.read_gray(os.path.join(dd, f)), io.read_gray(os.path.join(cd, f))
        h, w = min(px.shape[0], py.shape[0]), min(px.shape[1], py.shape[1])
        with torch.no_grad():
            out = m(io.to_input(px[:h, :w]).cuda(), io.to_input(py[:h, :w]).cuda())
        want = metrics.postprocess_u8(out[0, 0]).cpu().numpy()
        assert np.array_equal(io.read_gray(os.path.join(out_dir, f)), want), f

    # a checkpoint without EMA weights
    train.main(_cli(dd, cd, "--dtype", "f32", "--steps", "2", "--save", plain), emit=quiet)
    with pytest.raises(ValueError, match="plain.pth.*no EMA weights"):
        io.load_checkpoint(plain, CODONNet(), ema=True)
    with pytest.raises(ValueError, match="no EMA weights"):
        infer.main(["--weights", plain, "--ema", "--dtype", "f32", "--input-depth", dd, "--input-color", cd])

    # the same checkpoint as the options' predecessor wrote it: no new args keys, no new optimizer keys
    pk = torch.load(plain, weights_only=False)
    assert "model_ema" not in pk
    pk["args"] = {k: v for k, v in pk["args"].items() if k not in train.RESUME_DEFAULTS}
    pk["optimizer"] = {k: pk["optimizer"][k] for k in ("exp_avg", "exp_avg_sq", "t", "lr", "betas", "eps", "weight_decay")}
    assert sorted(pk["args"]) == ["batch", "crop", "dtype", "lr", "scale", "seed"]
    torch.save(pk, old)
    straight = train.main(_cli(dd, cd, "--dtype", "f32", "--steps", "3"), emit=quiet)
    resumed = train.main(_cli(dd, cd, "--dtype", "f32", "--steps", "3", "--resume", old), emit=quiet)
    assert resumed["losses"] == straight["losses"][2:] and "stats" not in resumed
    for p, q_ in zip(straight["gs"].params, resumed["gs"].params):
        assert torch.equal(p, q_)
    with pytest.raises(ValueError, match="other arguments"):
        train.main(_cli(dd, cd, "--dtype", "f32", "--steps", "3", "--resume", old, "--lr-schedule", "cosine"), emit=quiet)
