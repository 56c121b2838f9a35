"""A plain numpy restatement of what TaskPrompter/data/cityscapes3d.py:137-241 computes per frame, with Pillow's two resampling rules
written out (vectorised, independent of the loops in mtt_amd.cs3d).  tests/test_cs3d_host.py pins it to the reference's own outputs
(tests/golden/cs3d.*) and to PIL.Image.resize; the GPU tests then use it at shapes the fixture does not hold.

Pillow, Resample.c, 8-bit bilinear along one axis (in -> out): scale = in / out, filterscale = max(scale, 1), support = filterscale,
ksize = 2 * ceil(support) + 1; for output xx: center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0),
xmax = min(int(center + support + 0.5), in); w_x = tri((x + xmin - center + 0.5) / filterscale), divided by their sum; fixed to
int(0.5 + w * 2^22); one pass = clip8((2^21 + sum k * p) >> 22).  Horizontal first, rounded to uint8, then vertical; an axis of
unchanged size is skipped.
Pillow, Geometry.c, nearest along one axis: source index int(xo) with xo = 0.5 * in / out advanced by repeated ADDITION of in / out."""
import numpy as np

PRECISION_BITS = 22
VOID = [0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30]
VALID = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]
ORI_IMG_SIZE = (1024, 2048)


def bilinear_axis(n_in, n_out):
    """(first index int64 [n_out], tap count int64 [n_out], fixed-point weights int64 [n_out, ksize])"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    ksize = 2 * int(np.ceil(fs)) + 1
    center = (np.arange(n_out) + 0.5) * scale
    xmin = np.maximum((center - fs + 0.5).astype(np.int64), 0)              # astype truncates towards zero, as the C cast does
    xmax = np.minimum((center + fs + 0.5).astype(np.int64), n_in)
    cnt = xmax - xmin
    k = np.arange(ksize)
    arg = np.abs(((k[None, :] + xmin[:, None]) - center[:, None] + 0.5) * (1.0 / fs))
    w = np.where((arg < 1.0) & (k[None, :] < cnt[:, None]), 1.0 - arg, 0.0)
    ww = np.zeros(n_out)
    for j in range(ksize):                                                   # the sum in tap order, as the C loop accumulates it
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    return xmin, cnt, (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)     # the weights are >= 0: the -0.5 branch never applies


def _pass8(img, axis, n_out):
    """one 8-bit pass along `axis` of a uint8 array"""
    n_in = img.shape[axis]
    xmin, cnt, kk = bilinear_axis(n_in, n_out)
    a = np.moveaxis(img, axis, 0).astype(np.int64)
    acc = np.full((n_out,) + a.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for j in range(kk.shape[1]):
        src = np.minimum(xmin + j, n_in - 1)                                 # taps past the count have weight 0
        acc += kk[:, j].reshape((-1,) + (1,) * (a.ndim - 1)) * a[src]
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_bilinear_u8(img, size):
    """PIL.Image.fromarray(img).resize((size[1], size[0]), Image.BILINEAR) for uint8 [H, W] or [H, W, C]"""
    h, w = size
    out = img
    if w != img.shape[1]:
        out = _pass8(out, 1, w)
    if h != img.shape[0]:
        out = _pass8(out, 0, h)
    return out.copy() if out is img else out


def nearest_axis(n_in, n_out):
    step = n_in / n_out
    xo = np.cumsum(np.concatenate([[0.0 + step * 0.5], np.full(n_out - 1, step)]))       # cumsum adds in order: the recurrence
    return xo.astype(np.int64)


def nearest_axis_multiplied(n_in, n_out):
    """the obvious formula, which is NOT Pillow's: kept to show where the two part"""
    return ((np.arange(n_out) + 0.5) * n_in / n_out).astype(np.int64)


def resize_nearest(img, size):
    """PIL.Image.fromarray(img).resize((size[1], size[0]), Image.NEAREST) for [H, W] of any dtype"""
    h, w = size
    if (h, w) == img.shape[:2]:
        return img.copy()
    return img[nearest_axis(img.shape[0], h)][:, nearest_axis(img.shape[1], w)]


def encode_lut():
    lut = np.arange(256, dtype=np.int64)
    lut[VOID] = 255
    lut[VALID] = np.arange(19)
    return lut


def prepare_frame(image, labels, disparity, img_size, dd_label_map_size, mean, std, bgr=False, ori_img_size=ORI_IMG_SIZE):
    """one frame -> {'image' fp32 [3, h, w], 'semseg' int64 [h', w'], 'depth' fp32 [1, h', w'], 'flag' bool}; labels / disparity may be None"""
    rgb = image[..., ::-1] if bgr else image
    if tuple(img_size) != image.shape[:2]:
        rgb = resize_bilinear_u8(np.ascontiguousarray(rgb), img_size)
    t = rgb.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    out = {"image": (t - np.asarray(mean, np.float32)[:, None, None]) / np.asarray(std, np.float32)[:, None, None]}
    if labels is None:
        return out
    resample = tuple(dd_label_map_size) != tuple(ori_img_size)
    size = tuple(dd_label_map_size) if resample else labels.shape
    sem = encode_lut()[labels]
    sem = resize_nearest(sem, size)
    out["semseg"] = sem
    out["flag"] = bool(((sem != 255) & (sem >= 19)).any())
    if disparity is not None:
        d = disparity.astype(np.float32)
        d[d > 0] = (d[d > 0] - 1) / 256
        d[d == 0] = -1
        d[labels == 10] = 0                                                 # the RAW ids, before encode_segmap
        out["depth"] = resize_nearest(d, size)[None]
    return out


def prepare_batch(images, labels, disparities, prep):
    """the stacked batch a Cityscapes3DPrepare `prep` yields for stacked sources (numpy)"""
    frames = [prepare_frame(images[i], None if labels is None else labels[i], None if disparities is None else disparities[i], prep.img_size,
                            prep.dd_label_map_size, prep.mean, prep.std, bgr=prep.bgr, ori_img_size=prep.ori_img_size) for i in range(len(images))]
    out = {k: np.stack([f[k] for f in frames]) for k in frames[0] if k != "flag"}
    if labels is not None:
        out["flags"] = np.array([int(f["flag"]) for f in frames], dtype=np.int32)
    return out


def golden_sources(arrs, n=3):
    return [{k: arrs[f"src{j}_{k}"] for k in ("image", "semseg", "depth")} for j in range(n)]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()
