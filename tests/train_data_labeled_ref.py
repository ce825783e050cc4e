"""numpy restatement of the LABELED training-batch synthesis (codon_train_crops_labeled, codon_amd.train.synthesize on a
TrainSet with a label directory) -- TEST INFRASTRUCTURE; the three-plane companion of tests/train_data_ref.py, whose
definitions of the table, the D4 op, the downsample and the quantisation it uses unchanged.  The kernels must match it BIT
FOR BIT."""
import numpy as np

from oracle import upsample_oracle
from tests import train_data_ref as R


def crops(pool, descs, P):
    """(source, y, t): (B,1,P,P) fp32 each; descs rows = (pool offset, H, W, y0, x0, op); a record is depth map, guidance,
    label, each H*W bytes."""
    pool = np.asarray(pool, dtype=np.uint8)
    tab = R.lut()
    out = ([], [], [])
    for off, h, w, y0, x0, op in np.asarray(descs, dtype=np.int64).tolist():
        for k in range(3):
            plane = pool[off + k * h * w:off + (k + 1) * h * w].reshape(h, w)
            out[k].append(tab[R.d4(plane[y0:y0 + P, x0:x0 + P], op)])
    return tuple(np.stack(o)[:, None] for o in out)


def synthesize(pool, descs, s, P):
    """(x, y, t): x degraded from the depth plane, t from the label plane."""
    src, y, t = crops(pool, descs, P)
    x = R.quantize(upsample_oracle.bicubic_upsample(R.downsample(src, s), s))
    return x, y, t
