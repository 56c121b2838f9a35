"""TEST INFRASTRUCTURE ONLY — a numpy stand-in for the six names of OpenCV that the reference's data/transforms.py uses, so that the
unmodified file runs where OpenCV is absent (tests/golden/make_augment_golden.py puts this directory in front of sys.path).

It is written from OpenCV's documented algorithms with every operation and its order spelled out in fp32 / integer numpy; it is the
DEFINITION the HIP kernels of csrc/augment.hip mirror.  Parity of this file with a real OpenCV build (last ulp of the bilinear weights,
exact nearest-neighbour boundaries) is not pinned anywhere in this repository.

  resize INTER_NEAREST: sx = min(dx * src_w // dst_w, src_w - 1), the same along y
  resize INTER_LINEAR (float32 input): fx = float32((dx + 0.5) * (src / dst) - 0.5) with the product in fp64; sx = floor(fx), fx -= sx;
      sx < 0 -> (0, 0); sx >= src - 1 -> (src - 1, 0); second tap min(sx + 1, src - 1); a horizontal pass a0 * s0 + a1 * s1 with
      a0 = 1 - fx, a1 = fx, then the vertical pass on its result; every product and sum rounded to fp32
  cvtColor RGB2HSV (uint8, H in 0..179): integers, the reciprocal tables sdiv[i] = round(255 * 4096 / i), hdiv[i] = round(180 * 4096 /
      (6 i)) (half to even, entry 0 = 0), products shifted right by 12 after adding 2048
  cvtColor HSV2RGB (uint8): h = H * (6/180), s = S * (1/255), v = V * (1/255) in fp32, the sector table, the result * 255 rounded half to
      even and saturated
"""
import numpy as np

INTER_NEAREST = 0
INTER_LINEAR = 1
COLOR_RGB2HSV = 41
COLOR_HSV2RGB = 55

_SHIFT = 12
_f32 = np.float32


def _round_table(num):
    t = np.zeros(256, dtype=np.int64)
    i = np.arange(1, 256, dtype=np.float64)
    t[1:] = np.rint(num / i).astype(np.int64)
    return t


_SDIV = _round_table(float(255 << _SHIFT))
_HDIV = _round_table(float(180 << _SHIFT) / 6.0)
_SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])   # (b, g, r) <- tab[...]


def _linear_taps(src, dst):
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * (float(src) / float(dst)) - 0.5).astype(_f32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(_f32)).astype(_f32)
    low, high = s < 0, s >= src - 1
    s = np.where(low, 0, np.where(high, src - 1, s))
    f = np.where(low | high, _f32(0), f).astype(_f32)
    return s, np.minimum(s + 1, src - 1), (_f32(1) - f).astype(_f32), f


def resize(src, dsize, interpolation=INTER_LINEAR):
    src = np.asarray(src)
    dw, dh = int(dsize[0]), int(dsize[1])
    sh, sw = src.shape[:2]
    if interpolation == INTER_NEAREST:
        ys = np.minimum(np.arange(dh, dtype=np.int64) * sh // dh, sh - 1)
        xs = np.minimum(np.arange(dw, dtype=np.int64) * sw // dw, sw - 1)
        return np.ascontiguousarray(src[ys][:, xs])
    if interpolation != INTER_LINEAR or src.dtype != np.float32:
        raise NotImplementedError("stand-in: INTER_NEAREST, or INTER_LINEAR on float32")
    x0, x1, a0, a1 = _linear_taps(sw, dw)
    y0, y1, b0, b1 = _linear_taps(sh, dh)
    tail = (1,) * (src.ndim - 2)
    a0, a1 = a0.reshape((1, dw) + tail), a1.reshape((1, dw) + tail)
    b0, b1 = b0.reshape((dh, 1) + tail), b1.reshape((dh, 1) + tail)
    rows = (a0 * src[:, x0]).astype(_f32) + (a1 * src[:, x1]).astype(_f32)
    return ((b0 * rows[y0]).astype(_f32) + (b1 * rows[y1]).astype(_f32)).astype(_f32)


def _rgb2hsv(img):
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    v = np.maximum(r, np.maximum(g, b))
    diff = v - np.minimum(r, np.minimum(g, b))
    s = (diff * _SDIV[v] + (1 << (_SHIFT - 1))) >> _SHIFT
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * _HDIV[diff] + (1 << (_SHIFT - 1))) >> _SHIFT
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, np.minimum(s, 255), v], axis=-1).astype(np.uint8)


def _hsv2rgb(img):
    hi, si, vi = (img[..., k] for k in range(3))
    s = (si.astype(_f32) * (_f32(1) / _f32(255))).astype(_f32)
    v = (vi.astype(_f32) * (_f32(1) / _f32(255))).astype(_f32)
    h = (hi.astype(_f32) * (_f32(6) / _f32(180))).astype(_f32)
    sector = np.floor(h).astype(np.int64)
    h = (h - sector.astype(_f32)).astype(_f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, _f32(0), h).astype(_f32)
    one = _f32(1)
    tab = np.stack([v,
                    (v * (one - s)).astype(_f32),
                    (v * (one - (s * h).astype(_f32)).astype(_f32)).astype(_f32),
                    (v * (one - (s * (one - h).astype(_f32)).astype(_f32)).astype(_f32)).astype(_f32)], axis=-1)
    pick = _SECTOR[sector]                                                          # [..., 3] indices of (b, g, r)
    bgr = np.take_along_axis(tab, pick, axis=-1)
    grey = (si == 0)[..., None]
    bgr = np.where(grey, v[..., None], bgr).astype(_f32)
    out = np.clip(np.rint((bgr * _f32(255)).astype(_f32)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(out[..., ::-1])


def cvtColor(src, code):
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3:
        raise NotImplementedError("stand-in: 3-channel uint8 only")
    if code == COLOR_RGB2HSV:
        return _rgb2hsv(src)
    if code == COLOR_HSV2RGB:
        return _hsv2rgb(src)
    raise NotImplementedError("stand-in: COLOR_RGB2HSV and COLOR_HSV2RGB only")
