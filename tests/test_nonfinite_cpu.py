"""Non-finite inputs, the parts that need no GPU: the pin of what the REFERENCE does with a NaN / +Inf / -Inf pixel (run on
the float oracle, a restatement of the reference's forward), and the API surface of the guard.

What the reference does: torch's ReLU keeps NaN; the global average and max pools of the first CAC block
(CAC_module.py:43,47) spread it over every channel of that image; the gate (CODON_x4.py:89-91) multiplies it into every
pixel; the pools are per image, so the rest of the batch is untouched.  tests/test_gpu_nonfinite.py holds the HIP kernels to
this result in "propagate" mode."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import codon_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")


def _batch():
    g = torch.Generator().manual_seed(5)
    return torch.rand((3, 1, 24, 40), generator=g), torch.rand((3, 1, 24, 40), generator=g)


def _check(fwd, sd, x, y, clean, which, pos, val):
    px, py = x.clone(), y.clone()
    (px if which == "x" else py)[1, 0, pos[0], pos[1]] = val
    with torch.no_grad():
        out = fwd(sd, px, py)
    what = (which, pos, val)
    assert int(torch.isnan(out[1]).sum()) == 960, what          # all 960 elements of image 1
    assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2]), what     # bit-identical to the clean run


@pytest.mark.parametrize("variant", ["x4", "x16"])
def test_reference_pin_36_cases(variant):
    sd = orc.he_state(variant, 0)
    x, y = _batch()
    with torch.no_grad():
        clean = orc.forward(sd, x, y)
    assert bool(torch.isfinite(clean).all())
    n = 0
    for which in ("x", "y"):
        for pos in ((0, 0), (12, 20), (23, 39)):
            for val in (NAN, PINF, NINF):
                _check(orc.forward, sd, x, y, clean, which, pos, val)
                n += 1
    assert n == 18                                              # x 2 variants = the 36 cases


@pytest.mark.parametrize("fwd", ["forward_rmcr", "forward_cross"])
def test_reference_pin_ablation_nets(fwd):
    """The conv-only net has no global pool: its NaN region is the pixel's receptive field -- which at 24 x 40 is the image."""
    f = getattr(orc, fwd)
    sd = orc.he_state("x4", 0)
    x, y = _batch()
    with torch.no_grad():
        clean = f(sd, x, y)
    assert bool(torch.isfinite(clean).all())
    for val in (NAN, PINF):
        _check(f, sd, x, y, clean, "x", (12, 20), val)


def test_api_surface():
    import codon_amd
    from codon_amd import BaseNet_RMCR_fuseRMCR, BaseNet_RMCR_fuseRMCR_cross, CODONNet, CODONNet16, NonFiniteInputError
    assert issubclass(NonFiniteInputError, RuntimeError)
    e = NonFiniteInputError(True, False)
    assert e.depth is True and e.guidance is False and "depth" in str(e) and "guidance" not in str(e)
    assert "NonFiniteInputError" in codon_amd.__all__
    for cls in (CODONNet, CODONNet16, BaseNet_RMCR_fuseRMCR, BaseNet_RMCR_fuseRMCR_cross):
        m = cls()
        assert m.nonfinite_inputs == "raise"
        with pytest.raises(ValueError):
            m.set_nonfinite_inputs("bogus")
        for mode in ("propagate", "ignore", "raise"):
            assert m.set_nonfinite_inputs(mode) is m and m.nonfinite_inputs == mode
        assert m.check_inputs() is m and m.check_inputs(synchronize=False) is m      # nothing ran: nothing to report


def test_guard_state_is_dropped_by_pickle_and_deepcopy():
    import copy
    import io
    from codon_amd import CODONNet
    from codon_amd.model import _InputGuard
    m = CODONNet().set_nonfinite_inputs("propagate")
    m.__dict__["_iguard"] = _InputGuard()
    c = copy.deepcopy(m)
    assert c.__dict__.get("_iguard") is None and c.nonfinite_inputs == "propagate"
    assert m.__getstate__().get("_iguard") is None
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    r = torch.load(buf, weights_only=False)
    assert r.__dict__.get("_iguard") is None and r.nonfinite_inputs == "propagate"
    assert m.__dict__["_iguard"] is not None                    # the original keeps its own


def test_env_switch_makes_ignore_the_default():
    code = ("from codon_amd import CODONNet, BaseNet_RMCR_fuseRMCR; m = CODONNet(); "
            "assert m.nonfinite_inputs == 'ignore', m.nonfinite_inputs; "
            "assert BaseNet_RMCR_fuseRMCR().nonfinite_inputs == 'ignore'; "
            "assert m.set_nonfinite_inputs('raise').nonfinite_inputs == 'raise'; print('ok')")
    env = dict(os.environ, CODON_INPUT_GUARD="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_guarded_entries_validate_before_any_hip_call():
    """The guarded entry points keep the plain ones' argument validation (no GPU needed: it happens before any HIP call)."""
    from codon_amd import _lib
    lib = _lib.load()
    assert lib.codon_stem_fwd_guarded(1, 8, 8, None, None, None, 64, 0, _lib.F32, None, None, None) == -1
    assert b"null pointer" in lib.codon_last_error_string()
    assert lib.codon_head_fwd_guarded(1, 8, 8, None, 64, 0, None, None, None, _lib.F32, None, None) == -1
    assert lib.codon_head_fwd_y16_guarded(1, 8, 8, None, 64, 0, None, None, None, _lib.BF16, None, None) == -1
    assert lib.codon_stem_pair_fwd_guarded(1, 8, 8, None, None, None, 64, 0, None, None, None, 64, 0, _lib.F32, None, None,
                                           None, None) == -1
    assert lib.codon_weight_checksum_clear(None, None, None, 1, None, None, 0, None) == -1
