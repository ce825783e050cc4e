"""The host side of the guarded training step (gradient clipping, non-finite skipping, EMA, learning-rate schedules): the
schedule at closed-form points, every command-line refusal, unchanged defaults, the C ABI's refusals (host-side: no device is
touched) and the rule that no entry point of the library blocks or allocates."""
import ctypes as C
import glob
import math
import os
import re

import pytest

from codon_amd import train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--scale", "4", "--train-depth", "d", "--train-color", "c"]


def _close(a, b):
    return abs(a - b) <= 1e-15 * max(abs(a), abs(b))


def test_lr_at_closed_form_points():
    lr, lr_min, warmup, n = 3e-4, 1e-6, 10, 110
    at = lambda s, **kw: train.lr_at(s, **{"lr": lr, "schedule": "cosine", "warmup": warmup, "lr_min": lr_min, "lr_steps": n, **kw})  # noqa: E731
    assert _close(at(1), lr / warmup)
    assert _close(at(warmup), lr)
    assert _close(at(warmup + 1), lr_min + (lr - lr_min) * 0.5 * (1 + math.cos(math.pi / (n - warmup))))
    assert _close(at((warmup + n) // 2), (lr + lr_min) / 2)                      # the midpoint of the cosine
    assert all(at(s) == lr_min for s in (n, n + 1, n + 17, 10 * n))
    curve = [at(s) for s in range(1, n + 1)]
    assert all(a < b for a, b in zip(curve[:warmup - 1], curve[1:warmup]))       # up ...
    assert all(a > b for a, b in zip(curve[warmup - 1:-1], curve[warmup:]))      # ... then down
    assert all(isinstance(v, float) for v in curve)
    # no warm-up: the curve starts just below lr
    assert lr_min < at(1, warmup=0) < lr and at(n, warmup=0) == lr_min
    # constant: lr everywhere, a warm-up in front of it if asked for
    assert all(train.lr_at(s, lr=lr) == lr for s in (1, 2, 1000, 10 ** 9))
    assert _close(train.lr_at(3, lr=lr, warmup=4), lr * 3 / 4) and train.lr_at(5, lr=lr, warmup=4) == lr
    with pytest.raises(ValueError, match="schedule"):
        train.lr_at(1, lr=lr, schedule="linear")
    with pytest.raises(ValueError, match="lr_steps > warmup"):
        train.lr_at(11, lr=lr, schedule="cosine", warmup=10, lr_steps=10)


def test_cli_defaults_are_the_off_values():
    a = train.parse_args(BASE)
    assert (a.clip_norm, a.skip_nonfinite, a.ema, a.lr_schedule, a.warmup_steps, a.lr_min, a.lr_steps) == \
        (None, False, None, "constant", 0, 0.0, None)
    r = train.run_args(a)
    assert all(r[k] == train.RESUME_DEFAULTS[k] for k in train.RESUME_DEFAULTS)
    assert set(train.RESUME_DEFAULTS) < set(train.RESUME_KEYS) <= set(r)
    # the cosine curve's length resolves to --steps unless given
    a = train.parse_args(BASE + ["--lr-schedule", "cosine", "--steps", "50"])
    assert (a.lr_steps, a.lr_min) == (50, 0.0)
    a = train.parse_args(BASE + ["--lr-schedule", "cosine", "--steps", "50", "--lr-steps", "200", "--lr-min", "1e-6",
                                 "--warmup-steps", "60", "--clip-norm", "0.5", "--ema", "0.999", "--skip-nonfinite"])
    assert (a.lr_steps, a.lr_min, a.warmup_steps, a.clip_norm, a.ema, a.skip_nonfinite) == (200, 1e-6, 60, 0.5, 0.999, True)


@pytest.mark.parametrize("extra, message", [
    (["--clip-norm", "0"], "--clip-norm 0.0 must be positive"),
    (["--clip-norm", "-1"], "--clip-norm -1.0 must be positive"),
    (["--clip-norm", "nan"], "--clip-norm nan must be positive"),
    (["--ema", "1"], "--ema 1.0 must lie in [0, 1)"),
    (["--ema", "-0.1"], "--ema -0.1 must lie in [0, 1)"),
    (["--warmup-steps", "-1"], "--warmup-steps -1 must lie in [0, 1000)"),
    (["--warmup-steps", "20", "--steps", "20"], "--warmup-steps 20 must lie in [0, 20)"),
    (["--lr-schedule", "cosine", "--lr-steps", "8", "--warmup-steps", "8"], "--warmup-steps 8 must lie in [0, 8)"),
    (["--lr-schedule", "cosine", "--lr-min=-1e-6"], "--lr-min -1e-06 must lie in [0, --lr 0.0001]"),
    (["--lr-schedule", "cosine", "--lr-min", "1e-3"], "--lr-min 0.001 must lie in [0, --lr 0.0001]"),
    (["--lr-min", "1e-6"], "--lr-min and --lr-steps belong to --lr-schedule cosine"),
    (["--lr-steps", "100"], "--lr-min and --lr-steps belong to --lr-schedule cosine"),
    (["--lr-schedule", "cosine", "--lr-steps", "0"], "--lr-steps 0 must be positive"),
    (["--lr-schedule", "linear"], "invalid choice"),
])
def test_cli_refusals(capsys, extra, message):
    with pytest.raises(SystemExit) as e:
        train.parse_args(BASE + extra)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_resume_compares_missing_keys_as_defaults(tmp_path):
    """A checkpoint whose args predate the options resumes under the defaults and is refused under anything else."""
    import torch
    old = {"scale": 4, "crop": 32, "batch": 2, "dtype": "bf16", "lr": 1e-4, "seed": 0}
    path = str(tmp_path / "old.pth")
    torch.save({"epoch": 1, "model": {}, "optimizer": {}, "rng": {}, "args": old}, path)
    now = train.run_args(train.parse_args(BASE + ["--crop", "32", "--batch", "2"]))
    assert train.load_resume(path, now)["epoch"] == 1
    for extra in (["--lr-schedule", "cosine"], ["--clip-norm", "1"], ["--skip-nonfinite"], ["--ema", "0.9"], ["--warmup-steps", "3"]):
        now = train.run_args(train.parse_args(BASE + ["--crop", "32", "--batch", "2"] + extra))
        with pytest.raises(ValueError, match="other arguments"):
            train.load_resume(path, now)


def guarded_refusals(lib, ptr, L):
    """Every refusal of codon_grad_norm / codon_adam_step_guarded, all decided on the host before any launch; `ptr` stands for
    every buffer (a fake address without a GPU, a real allocation with one).  Shared with tests/test_gpu_guarded_step.py."""
    inf = float("inf")

    def desc(n=1, count=1024, param=ptr):
        d = L.AdamDesc()
        d.n = n
        for i in range(max(0, min(n, L.ADAM_MAX))):
            d.param[i], d.count[i] = param.value, count
        return d

    def step(d=None, grad=ptr, m=ptr, v=ptr, ema=None, state=ptr, max_norm=1.0, decay=0.0, t=1, null_desc=False):
        d = desc() if d is None else d
        st = lib.codon_adam_step_guarded(None if null_desc else C.byref(d), grad, m, v, ema, state, 1e-3, 0.9, 0.999, 1e-8, 0.0, t,
                                         max_norm, 1, decay, None)
        return st, lib.codon_last_error_string().decode()

    assert lib.codon_grad_norm_workspace_bytes() >= 4 * 8
    for kw in ({"null_desc": True}, {"grad": None}, {"m": None}, {"v": None}, {"state": None}):
        assert step(**kw) == (-1, "adam_step_guarded: null pointer"), kw
    for bad in (0.0, -1.0, -inf, float("nan")):
        st, msg = step(max_norm=bad)
        assert st == -1 and msg.startswith("adam_step_guarded: max_norm"), (bad, msg)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        st, msg = step(ema=ptr, decay=bad)
        assert st == -1 and msg.startswith("adam_step_guarded: EMA decay"), (bad, msg)
    for n in (0, -1, L.ADAM_MAX + 1):
        st, msg = step(d=desc(n=n), max_norm=inf)
        assert st == -1 and "tensors (1.." in msg, (n, msg)
    st, msg = step(d=desc(count=0))
    assert st == -1 and "null, empty or misaligned" in msg
    st, msg = step(d=desc(n=2, count=1 << 31))
    assert st == -2 and "too many elements" in msg
    assert step(t=0)[0] == -1
    assert step(state=C.c_void_p(ptr.value + 4))[0] == -1                     # the state block holds 8-byte words
    for args in ((None, 8, ptr), (ptr, 8, None)):
        assert lib.codon_grad_norm(*args, None) == -1 and lib.codon_last_error_string() == b"grad_norm: null pointer"
    for n in (0, -5, 1 << 32):
        assert lib.codon_grad_norm(ptr, n, ptr, None) == -1 and b"elements" in lib.codon_last_error_string(), n
    assert lib.codon_grad_norm(C.c_void_p(ptr.value + 4), 8, ptr, None) == -1 and b"aligned" in lib.codon_last_error_string()


def test_guarded_step_refusals_without_gpu():
    from codon_amd import _lib as L
    guarded_refusals(L.load(), C.c_void_p(4096), L)      # never dereferenced: every call is refused on the host


def test_no_entry_point_blocks_or_allocates():
    """The library only launches: no stream / device synchronise, no memcpy, no allocation anywhere in csrc (a training step
    stays free of host synchronisation only as long as this holds)."""
    files = sorted(glob.glob(os.path.join(ROOT, "codon_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "codon_amd", "csrc", "*.h")))
    assert len(files) >= 18
    banned = re.compile(r"\bhip\w*Synchronize\w*|\bhipMemcpy\w*|\bhipMalloc\w*|\bhipFree\w*")
    hits = []
    for f in files:
        src = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(f).read(), flags=re.S)          # comments may speak of them
        hits += [(os.path.basename(f), m.group(0)) for m in banned.finditer(src)]
    assert not hits, hits
