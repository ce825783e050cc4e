"""Fixed inputs for the loss and metrics kernels and SHA-256 digests of what the public API returns for them
(tests/test_gpu_metrics_bits.py).  The inputs come from integer arithmetic alone -- a multiplicative hash of the
pixel index, reduced to 16 bits, divided by 65535 in float32 -- so they are the same on any machine and any torch version.
Only the public names of codon_amd.metrics are called: the module runs unchanged on an older tree, which is how
tests/golden/metrics_bits.json is recorded (python -m tests.metrics_bits OUT.json, on the commit BEFORE a change)."""
import hashlib
import json
import sys

import numpy as np
import torch

UNMASKED = [(1, 7, 7), (3, 9, 70), (1, 33, 64), (2, 40, 52)]
MASKED = [(5, 37, 53), (1, 128, 128), (1, 370, 463)]
W_L1, W_SSIM = 1.0, 0.7


def hash16(n, salt):
    """16 hashed bits per index 0 .. n-1 as int64."""
    h = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = h * np.uint64(2246822519) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    return ((h >> np.uint64(8)) & np.uint64(0xFFFF)).astype(np.int64)


def images(B, H, W):
    """p, t codes (int64, 1 .. 65535) of shape (B,1,H,W): t is p moved by up to +-4096 codes (0 at some pixels)."""
    n = B * H * W
    p = np.maximum(hash16(n, 1), 1)
    t = np.clip(p + hash16(n, 2 * n + 7) % 8192 - 4096, 1, 65535)
    return p.reshape(B, 1, H, W), t.reshape(B, 1, H, W)


def mask(B, H, W):
    """bool (B,1,H,W): a hole where the hash is below 3 %, plus one rectangle per image; with B >= 5 image 3 has a hole every
    fifth pixel both ways (e_b = 0, n_b > 0) and image 4 is all invalid (n_b = 0)."""
    v = (hash16(B * H * W, 5 * B * H * W + 11) >= 1966).reshape(B, 1, H, W)
    v[:, :, H // 3:H // 3 + max(2, H // 6), W // 4:W // 4 + max(2, W // 5)] = False
    if B >= 5:
        v[3] = True
        v[3, 0, ::5, ::5] = False
        v[4] = False
    return v


def as_f32(codes):
    return torch.from_numpy(codes.astype(np.float32) / np.float32(65535)).cuda()


def sqerr_planes(bits):
    """label, out codes (int64, (37, 53)) of the given width; about 3 % of the label is 0; the 16-bit pair holds 65535 against 0
    both ways round at valid pixels, so that d * d needs more than 31 bits."""
    H, W, top = 37, 53, (1 << bits) - 1
    label = hash16(H * W, 21) >> (16 - bits)
    out = hash16(H * W, 22) >> (16 - bits)
    label[hash16(H * W, 23) < 1966] = 0
    label, out = label.reshape(H, W), out.reshape(H, W)
    label[1, 1], out[1, 1] = top, 0
    label[2, 2], out[2, 2] = 1, top
    label[3, 3], out[3, 3] = 0, top
    return label, out


def sqerr_closed_form(label, out):
    m = label != 0
    return int(((label - out)[m] ** 2).sum()), int(m.sum())


def sqerr(bits):
    """-> (sum of squared errors, count) from the device kernel, as Python ints."""
    from codon_amd import metrics
    label, out = sqerr_planes(bits)
    if bits == 8:
        acc = metrics.masked_sqerr_dev(torch.from_numpy(label.astype(np.uint8)).cuda(),
                                       torch.from_numpy(out.astype(np.uint8)).cuda())
    else:
        acc = metrics.masked_sqerr_u16_dev(torch.from_numpy(label.astype(np.uint16)).cuda(),
                                           torch.from_numpy(out.astype(np.uint16)).cuda())
    return tuple(int(v) for v in acc.cpu())


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def digests():
    """{case: sha256 of the raw little-endian bytes of the output}."""
    from codon_amd import metrics
    d = {}
    for B, H, W in UNMASKED:
        k = f"l1ssim_{B}x{H}x{W}"
        pc, tc = images(B, H, W)
        p, t = as_f32(pc).requires_grad_(True), as_f32(tc)
        loss = metrics.L1SSIMLoss(W_L1, W_SSIM)(p, t)
        loss.backward()
        d[k + "_value"], d[k + "_grad"] = _sha(loss), _sha(p.grad)
        d[f"ssim_dev_{B}x{H}x{W}"] = _sha(metrics.ssim_dev(p.detach(), t))
    for B, H, W in MASKED:
        pc, tc = images(B, H, W)
        v = mask(B, H, W)
        for explicit in (True, False):
            # valid=None reads the holes off the target: codes are >= 1, so t == 0 exactly where the mask says
            t = as_f32(tc if explicit else np.where(v, tc, 0))
            vd = torch.from_numpy(v.astype(np.uint8)).cuda() if explicit else None
            k = f"masked_{'mask' if explicit else 'none'}_{B}x{H}x{W}"
            d[k + "_counts"] = _sha(metrics.masked_counts(t, vd))
            for up in (1.0, -2.0):
                p = as_f32(pc).requires_grad_(True)
                loss = metrics.MaskedL1SSIMLoss(W_L1, W_SSIM)(p, t, vd)
                (loss * up).backward()
                d[f"{k}_up{up:g}_value"], d[f"{k}_up{up:g}_grad"] = _sha(loss), _sha(p.grad)
    for bits in (8, 16):
        d[f"sqerr_u{bits}"] = _sha(torch.tensor(sqerr(bits), dtype=torch.int64))
    return d


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(digests(), f, indent=1, sort_keys=True)
        f.write("\n")
