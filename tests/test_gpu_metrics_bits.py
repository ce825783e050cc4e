"""The loss and metrics kernels return the bits they returned before csrc/metrics.hip was folded onto one SSIM tile body, one
backward body and one masked squared-error kernel.  tests/golden/metrics_bits.json was recorded with
tests/metrics_bits.py on the commit before that change, on an MI355X; every digest must match -- the kernels use no
floating-point atomics, so there is nothing to exclude."""
import json
import os

import pytest

from tests import metrics_bits as MB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "metrics_bits.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def digests():
    return MB.digests()


def test_same_cases_as_the_golden(golden, digests):
    assert sorted(digests) == sorted(golden)


def _cases():
    c = []
    for B, H, W in MB.UNMASKED:
        c += [f"l1ssim_{B}x{H}x{W}_value", f"l1ssim_{B}x{H}x{W}_grad", f"ssim_dev_{B}x{H}x{W}"]
    for B, H, W in MB.MASKED:
        for m in ("mask", "none"):
            k = f"masked_{m}_{B}x{H}x{W}"
            c += [k + "_counts"] + [f"{k}_up{up}_{what}" for up in ("1", "-2") for what in ("value", "grad")]
    return c + ["sqerr_u8", "sqerr_u16"]


@pytest.mark.parametrize("case", _cases())
def test_bits_are_the_parent_commits(golden, digests, case):
    assert digests[case] == golden[case]


@pytest.mark.parametrize("bits", [8, 16])
def test_masked_sqerr_is_the_closed_form_sum(bits):
    label, out = MB.sqerr_planes(bits)
    want = MB.sqerr_closed_form(label, out)
    if bits == 16:
        assert ((label - out)[label != 0] ** 2).max() == 65535 ** 2 > 2 ** 31
    assert (label == 0).any()
    assert MB.sqerr(bits) == want
