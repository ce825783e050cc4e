"""Image / checkpoint plumbing of the reference script, host side only:
   PNG -> grey uint8 -> /255 -> (1,1,H,W) float32      /root/reference/CODON_X4/test.py:116-123
   {"epoch", "model": <nn.Module>} pickles and 'module.'-prefixed state dicts      test.py:56-59, CODON_X16/test.py:52-60

Grey conversion: the reference uses cv2.imread(name, 0); OpenCV is absent here, PIL's convert('L') is used
instead (ITU-R 601 weights, may differ from OpenCV by +-1 on colour images) -- PARITY UNPINNED for RGB inputs;
single-channel PNGs (all depth maps and labels) are read identically."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch


def read_gray(path: str) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"), dtype=np.uint8)


def write_gray(path: str, img_u8: np.ndarray):
    from PIL import Image
    Image.fromarray(np.asarray(img_u8, dtype=np.uint8), mode="L").save(path)


DEPTH16_MODES = ("I;16", "I;16B", "I;16L", "I")


def read_depth(path: str) -> np.ndarray:
    """A depth map or label with its own bit depth: uint16 codes for PIL's 16-bit greyscale modes (I;16, I;16B, I;16L) and for
    mode I (32-bit integers, refused if a value lies outside [0, 65535]); uint8 exactly as read_gray for everything else.
    convert("L") CLIPS a 16-bit image at 255, which is why read_gray must not be used on one."""
    from PIL import Image
    im = Image.open(path)
    if im.mode not in DEPTH16_MODES:
        return np.asarray(im.convert("L"), dtype=np.uint8)
    a = np.asarray(im)
    if im.mode == "I" and a.size and (int(a.min()) < 0 or int(a.max()) > 65535):
        raise ValueError(f"{path}: mode I image with values outside [0, 65535] (min {int(a.min())}, max {int(a.max())})")
    return np.ascontiguousarray(a.astype(np.uint16))


def write_depth16(path: str, arr_u16: np.ndarray):
    """A 16-bit greyscale PNG of uint16 codes."""
    from PIL import Image
    a = np.ascontiguousarray(np.asarray(arr_u16, dtype=np.uint16))
    Image.frombytes("I;16", (a.shape[1], a.shape[0]), a.astype("<u2").tobytes()).save(path)


def check_depth_max(depth_max):
    if not isinstance(depth_max, (int, np.integer)) or not 1 <= depth_max <= 65535:
        raise ValueError(f"depth_max {depth_max!r} must be an integer in [1, 65535]")


def read_depth_plane(path: str, depth_bits: int, depth_max: int = 65535) -> np.ndarray:
    """One depth map or label under the data set's bit depth: 8 -> read_gray's uint8, and a 16-bit file is
    REFUSED (convert("L") would clip it at 255 without a word); 16 -> uint16 codes, an 8-bit file refused (no mixing) and so
    is a code above depth_max.  Every ValueError names the file."""
    a = read_depth(path)
    if depth_bits == 8:
        if a.dtype != np.uint8:
            raise ValueError(f"{path}: a 16-bit image (codes up to {int(a.max())}) in an 8-bit data set; it would be clipped at "
                             "255 -- pass --depth-bits 16 (and --depth-max)")
        return a
    if a.dtype != np.uint16:
        raise ValueError(f"{path}: an 8-bit image in a 16-bit data set (--depth-bits 16): depth maps and labels must all be "
                         "16-bit")
    if a.size and int(a.max()) > depth_max:
        raise ValueError(f"{path}: code {int(a.max())} lies above depth_max {depth_max}")
    return a


def list_pairs(input_depth: str, input_color: str):
    return [f for f in sorted(os.listdir(input_color)) if os.path.exists(os.path.join(input_depth, f))]


def to_input(pic_u8: np.ndarray) -> torch.Tensor:
    """torch.from_numpy(pic / 255).float().unsqueeze(0).unsqueeze(0)   (float64 divide, then float32)."""
    return torch.from_numpy(np.asarray(pic_u8) / 255).float().unsqueeze(0).unsqueeze(0)


def _compat_on_path():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "compat")
    if d not in sys.path:
        sys.path.insert(0, d)


def load_checkpoint(path: str, model: torch.nn.Module, strict: bool = True, ema: bool = False) -> int:
    """Load the reference's checkpoint formats into `model`; returns the stored epoch (or -1).
    Whole-module pickles name the classes CODON_x4.CODONNet / CAC_module.*: codon_amd/compat provides them.
    ema: load "model_ema" (the EMA weights a `codon_amd.train --ema` checkpoint carries) instead of "model"."""
    from .model import strip_module_prefix
    _compat_on_path()
    ck = torch.load(path, map_location="cpu", weights_only=False)
    epoch = -1
    if ema and not (isinstance(ck, dict) and "model_ema" in ck):
        raise ValueError(f"{path}: the checkpoint holds no EMA weights (\"model_ema\": written by codon_amd.train --ema)")
    if isinstance(ck, dict) and "model" in ck:
        epoch = int(ck.get("epoch", -1))
        ck = ck["model_ema" if ema else "model"]
    sd = ck.state_dict() if isinstance(ck, torch.nn.Module) else ck
    model.load_state_dict(strip_module_prefix(sd), strict=strict)
    return epoch
