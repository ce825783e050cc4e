"""CPU pins of the hole-aware loss's yardstick (tests/masked_loss_ref.py, the float64 restatement the GPU tests compare the
kernels with): all-valid it is the metrics oracle's ssim_exact and mean|p - t|; its counts are a brute-force numpy count on
crops of shipped labels (tests/golden/metrics_crops.npz: Books and Dolls carry holes); holes carry nothing.  No GPU."""
import os

import numpy as np
import pytest
import torch

from oracle import metrics_oracle as mo
from tests import masked_loss_ref as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_crops.npz")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLD)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))[None, None]


@pytest.mark.parametrize("name", ["Art", "Books", "Dolls"])
def test_all_valid_is_ssim_exact_and_mean_abs(z, name):
    out, lab = z[f"{name}.output"] / 255.0, z[f"{name}.label"] / 255.0
    ones = torch.ones(1, 1, *out.shape, dtype=torch.uint8)
    l1, s, n, e = M.terms(_t(out), _t(lab), ones)
    assert int(n) == int(e) == out.size
    assert abs(float(s) - mo.ssim_exact(out, lab)) < 1e-12
    assert abs(float(s) - float(z[f"{name}.ssim_out_label"])) < 1e-12          # the value recorded from the reference's ssim_2
    assert abs(float(l1) - float(np.abs(out - lab).mean())) < 1e-15
    full = M.masked_loss(_t(out), _t(lab), ones, 1.0, 0.7)
    assert abs(float(full) - (np.abs(out - lab).mean() + 0.7 * (1 - mo.ssim_exact(out, lab)))) < 1e-12


@pytest.mark.parametrize("name", ["Art", "Books", "Dolls"])
def test_counts_equal_brute_force_on_shipped_labels(z, name):
    lab = z[f"{name}.label"]
    holes = int((lab == 0).sum())
    assert holes == {"Art": 0, "Books": 10, "Dolls": 96}[name]
    got = M.counts(_t(lab)).numpy()
    want = M.counts_brute(lab[None, None])
    assert np.array_equal(got, want), (got, want)
    assert got[0, 0] == lab.size - holes and (got[0, 1] < got[0, 0]) == (holes > 0)


def test_counts_with_explicit_mask_and_borders():
    """A hole in a corner is seen several times by the reflected windows around it; an explicit mask overrides t != 0."""
    g = np.random.default_rng(3)
    t = g.uniform(0.1, 1, (2, 1, 20, 17))
    v = np.ones(t.shape, dtype=np.uint8)
    v[0, 0, 0, 0] = 0
    v[1, 0, 9:12, 5:7] = 0
    v[1, 0, 19, 16] = 0
    got = M.counts(torch.from_numpy(t), torch.from_numpy(v)).numpy()
    assert np.array_equal(got, M.counts_brute(t, v))
    assert got[0].tolist() == [20 * 17 - 1, 20 * 17 - 49]                      # the 7x7 pixels whose window reaches (0, 0)
    assert np.array_equal(M.counts(torch.from_numpy(t)).numpy(), [[340, 340], [340, 340]])


def test_holes_carry_no_loss_and_no_gradient():
    g = np.random.default_rng(4)
    p = g.uniform(0, 1, (3, 1, 30, 33))
    t = np.clip(p + g.normal(0, 0.1, p.shape), 0.01, 1)
    v = g.uniform(size=p.shape) > 0.02
    v[0, 0, 4:12, 6:20] = False
    v[1] = False                                                              # n_b = 0: contributes nothing
    v[2, 0, ::5, ::5] = False                                                 # e_b = 0, n_b > 0: the L1 term alone
    vt = torch.from_numpy(v)
    pt = torch.from_numpy(p).requires_grad_(True)
    loss = M.masked_loss(pt, torch.from_numpy(t), vt)
    loss.backward()
    l1, s, n, e = M.terms(torch.from_numpy(p), torch.from_numpy(t), vt)
    assert n.tolist()[1] == 0 and e.tolist()[1] == 0 and e.tolist()[2] == 0 and n.tolist()[2] > 0 and e.tolist()[0] > 0
    assert float(l1[1]) == 0 and s.tolist()[1:] == [1.0, 1.0]
    assert abs(float(loss.detach()) - float((l1[0] + 1 - s[0] + l1[2]) / 3)) < 1e-15
    assert (pt.grad[~vt] == 0).all() and (pt.grad[1] == 0).all() and torch.isfinite(pt.grad).all()
    # other values in the holes, NaN and Inf included, change nothing
    for junk in (7.5, float("nan"), float("inf"), -float("inf")):
        p2, t2 = p.copy(), t.copy()
        p2[~v], t2[~v] = junk, -junk if junk == junk else junk
        q = torch.from_numpy(p2).requires_grad_(True)
        l2 = M.masked_loss(q, torch.from_numpy(t2), vt)
        l2.backward()
        assert float(l2.detach()) == float(loss.detach()) and torch.equal(q.grad, pt.grad)
    # valid = None is t != 0
    t0 = np.where(v, t, 0.0)
    assert float(M.masked_loss(torch.from_numpy(p), torch.from_numpy(t0))) == float(loss.detach())


def test_per_image_means_make_shards_consistent():
    g = np.random.default_rng(5)
    p, t = g.uniform(0, 1, (4, 1, 24, 24)), g.uniform(0.05, 1, (4, 1, 24, 24))
    v = torch.from_numpy(g.uniform(size=p.shape) > 0.01)
    v[3, 0, :, :12] = False
    P, T = torch.from_numpy(p), torch.from_numpy(t)
    whole = M.masked_loss(P, T, v)
    halves = (M.masked_loss(P[:2], T[:2], v[:2]) + M.masked_loss(P[2:], T[2:], v[2:])) / 2
    assert abs(float(whole) - float(halves)) < 1e-15
