"""float64 torch restatement of the hole-aware L1 + SSIM loss (codon_amd.metrics.MaskedL1SSIMLoss) and a
brute-force numpy count of {n_b, e_b} -- TEST INFRASTRUCTURE, the yardstick of tests/test_gpu_masked_loss.py.  Pinned on the CPU
by tests/test_masked_loss_cpu.py: with an all-ones mask its SSIM term is the metrics oracle's ssim_exact (1e-12) and its L1
term mean|p - t|.

    v    validity: the caller's mask (nonzero = valid) or t != 0
    E_b  pixels whose whole 13x13 window is valid under scipy-'reflect' indexing
    loss = (1/B) sum_b [ w_l1 * sum_v |p - t| / max(n_b, 1) + w_ssim * (1 - SSIM_b) ],
    SSIM_b = sum_{E_b} ssim / e_b, 1 when e_b = 0;  invalid pixels of p and t read as 0."""
import numpy as np
import torch

from oracle import metrics_oracle as mo

R = 6                                                    # radius of the 13-tap Gaussian (sd 1.5, truncate 4.0)


def _index(n):
    return mo._reflect_index(n, R)


def _filter(x, w):
    """Separable 13-tap filter with reflect boundary over the last two axes (rows first, as metrics_oracle.ssim_torch)."""
    H, W = x.shape[-2:]
    iy, ix = _index(H), _index(W)
    xp = x[..., iy, :]
    x = sum(w[k] * xp[..., k:k + H, :] for k in range(len(w)))
    xp = x[..., :, ix]
    return sum(w[k] * xp[..., :, k:k + W] for k in range(len(w)))


def ssim_map(a, b, C1=0.01 ** 2, C2=0.03 ** 2):
    """Per-pixel SSIM of (B,1,H,W) float64 tensors: ssim_exact's expression before its mean."""
    w = torch.from_numpy(mo.gauss_weights(1.5)).to(a.dtype)
    G = lambda x: _filter(x, w)                            # noqa: E731
    mu1, mu2 = G(a), G(b)
    s1, s2, s12 = G(a * a) - mu1 * mu1, G(b * b) - mu2 * mu2, G(a * b) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def validity(t, valid=None):
    return (t != 0) if valid is None else (valid != 0)


def window_valid(v):
    """E: (B,1,H,W) bool -- no invalid pixel in the 13x13 reflect-indexed window."""
    bad = _filter((~v).to(torch.float64), torch.ones(2 * R + 1, dtype=torch.float64))
    return bad == 0


def counts(t, valid=None):
    """(B,2) int64 {n_b, e_b}."""
    v = validity(t, valid)
    return torch.stack([v.flatten(1).sum(1), window_valid(v).flatten(1).sum(1)], dim=1)


def terms(p, t, valid=None):
    """(L1_b, SSIM_b, n_b, e_b): per-image float64 tensors of shape (B,)."""
    v = validity(t, valid)
    zero = torch.zeros((), dtype=p.dtype)
    p0, t0 = torch.where(v, p, zero), torch.where(v, t, zero)
    E = window_valid(v)
    n, e = v.flatten(1).sum(1), E.flatten(1).sum(1)
    l1 = torch.where(v, (p0 - t0).abs(), zero).flatten(1).sum(1) / n.clamp(min=1)
    s = torch.where(E, ssim_map(p0, t0), zero).flatten(1).sum(1) / e.clamp(min=1)
    s = torch.where(e > 0, s, torch.ones_like(s))
    return l1, s, n, e


def masked_loss(p, t, valid=None, w_l1=1.0, w_ssim=1.0):
    """The loss as a float64 scalar; differentiable in p."""
    l1, s, _, _ = terms(p, t, valid)
    return (w_l1 * l1 + w_ssim * (1 - s)).mean()


def counts_brute(t, valid=None):
    """numpy, no filter: pad the validity symmetrically by 6 and look at every 13x13 window."""
    t = np.asarray(t)
    v = (t != 0) if valid is None else (np.asarray(valid) != 0)
    out = []
    for vb in v.reshape(-1, *v.shape[-2:]):
        H, W = vb.shape
        pad = np.pad(vb, R, mode="symmetric")
        e = sum(int(pad[i:i + 2 * R + 1, j:j + 2 * R + 1].all()) for i in range(H) for j in range(W))
        out.append((int(vb.sum()), e))
    return np.asarray(out, dtype=np.int64)
