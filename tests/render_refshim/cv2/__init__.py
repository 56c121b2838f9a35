"""TEST INFRASTRUCTURE ONLY — the three names of OpenCV that the reference's utils/visualization_utils.py and
evaluation/evaluate_utils.py use on the way to a file, so that the unmodified files run where OpenCV is absent
(tests/golden/make_render_golden.py puts this directory in front of sys.path).  Nothing is encoded or written:

  imwrite(path, arr)             records (path, a copy of arr) in CAPTURED
  applyColorMap(idx, colormap)   records the uint8 index array in INDEXED and returns it stacked three times along a new last axis
                                 (OpenCV's COLORMAP_JET table is not available here, so the colours themselves are not pinned)
"""
import threading

import numpy as np

COLORMAP_JET = 2
CAPTURED, INDEXED = [], []
_LOCK = threading.Lock()


def imwrite(path, arr):
    with _LOCK:
        CAPTURED.append((str(path), np.array(arr)))
    return True


def applyColorMap(idx, colormap):
    if colormap != COLORMAP_JET or idx.dtype != np.uint8 or idx.ndim != 2:
        raise NotImplementedError("stand-in: COLORMAP_JET on a uint8 [H, W] index")
    with _LOCK:
        INDEXED.append(np.array(idx))
    return np.stack([idx, idx, idx], axis=-1)
