"""TEST INFRASTRUCTURE ONLY — the four names of OpenCV that the reference's data/cityscapes3d.py uses, over Pillow's PNG decoder, so
that the unmodified file runs where OpenCV is absent (tests/golden/make_cs3d_golden.py puts this directory in front of sys.path).

  imread(path)                     an 8-bit colour PNG as uint8 [H, W, 3] in B, G, R order
  imread(path, IMREAD_UNCHANGED)   the file's own depth and channels: a 16-bit grey PNG as uint16 [H, W]
  cvtColor(img, COLOR_BGR2RGB)     the channel axis reversed
"""
import numpy as np
from PIL import Image

IMREAD_UNCHANGED = -1
COLOR_BGR2RGB = 4


def imread(path, flags=1):
    im = Image.open(path)
    if flags == IMREAD_UNCHANGED:
        a = np.array(im)
        return a[..., ::-1].copy() if a.ndim == 3 else a
    return np.array(im.convert("RGB"))[..., ::-1].copy()


def cvtColor(img, code):
    if code != COLOR_BGR2RGB:
        raise NotImplementedError(code)
    return np.ascontiguousarray(img[..., ::-1])
