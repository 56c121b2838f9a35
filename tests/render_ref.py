"""An fp64 numpy restatement of what the reference does to a prediction before it is encoded into a file: the interpolation, the
get_output rules, the truncation, the colour tables, the centre crop and the skip rule.  tests/test_render_host.py pins it to the
unmodified reference (tests/golden/render.*); tests/test_gpu_render.py judges the device against it.

How bytes are judged.  The device and the reference's CPU torch both work in fp32, in different orders, so a byte is
decided where a value crosses an integer and a class where two logits meet:
  * a byte pixel is LEFT OUT when its fp64 value lies within delta of an integer without being one; it may then differ by one level;
  * an arg-max pixel is LEFT OUT when its two largest interpolated logits lie within delta of each other (and differ); it may then be
    the runner-up class;
  * everywhere else the bytes must be equal.  Exact integers (the zeros of a clamped depth map, each image's minimum and maximum pixel)
    and exact ties are judged, never left out.  At identity size the interpolated values are the source values, so classes and fp32
    depth compare with == and nothing is left out."""
import numpy as np

CAP = 0.05                              # the largest share of a case that may be left out


# ---- interpolation: F.interpolate(x, size, mode='bilinear'), align_corners=False ------------------------------------------------------------
def taps(n_in, n_out):
    """PyTorch's area_pixel_compute_source_index + guard_index_and_lambda in the fp32 it uses: (i0, i1, lambda as fp64 of the fp32 value)"""
    f32 = np.float32
    scale = f32(n_in) / f32(n_out)
    s = (scale * (np.arange(n_out, dtype=np.float32) + f32(0.5))).astype(np.float32) - f32(0.5)
    s = np.maximum(s, f32(0)).astype(np.float32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    lam = np.clip((s - i0.astype(np.float32)).astype(np.float32), f32(0), f32(1))
    return i0, np.minimum(i0 + 1, n_in - 1), lam.astype(np.float64)


def interpolate(x, size, rows=None, cols=None):
    """x [B, C, h, w] -> fp64 [B, C, H, W]; the horizontal pair first, then the vertical one (UpSampleKernel.cpp's nested interpolate).
    Equal sizes return the source values themselves.  rows / cols: only these output rows / columns (a sample of a large frame)."""
    x = np.asarray(x, dtype=np.float64)
    H, W = int(size[0]), int(size[1])
    rows = np.arange(H) if rows is None else np.asarray(rows)
    cols = np.arange(W) if cols is None else np.asarray(cols)
    if x.shape[2:] == (H, W):
        return x if len(rows) == H and len(cols) == W else x[:, :, rows][:, :, :, cols]
    y0, y1, ly = (a[rows] for a in taps(x.shape[2], H))
    x0, x1, lx = (a[cols] for a in taps(x.shape[3], W))
    top, bottom = x[:, :, y0], x[:, :, y1]
    ly = ly[:, None]
    return (top[..., x0] * (1.0 - lx) + top[..., x1] * lx) * (1.0 - ly) + (bottom[..., x0] * (1.0 - lx) + bottom[..., x1] * lx) * ly


# ---- get_output (TaskPrompter/utils/utils.py:27-63) -------------------------------------------------------------------------------------------
def top2(v):
    """arg-max over C, the first index winning ties (utils.py:33-43): (index, runner-up index, gap >= 0).  One class: runner-up = index."""
    idx = np.argmax(v, axis=1)
    if v.shape[1] == 1:
        return idx, idx, np.full(idx.shape, np.inf)
    best = np.take_along_axis(v, idx[:, None], axis=1)[:, 0]
    rest = v.copy()
    np.put_along_axis(rest, idx[:, None], -np.inf, axis=1)
    run = np.argmax(rest, axis=1)
    return idx, run, best - np.take_along_axis(rest, run[:, None], axis=1)[:, 0]


def sigmoid255(v):
    """edge (utils.py:45-47): 255 * 1 / (1 + exp(-x))"""
    return 255.0 / (1.0 + np.exp(-v[:, 0]))


def softmax1_255(v):
    """sal (utils.py:49-51): softmax over C, channel 1, * 255"""
    e = np.exp(v - v.max(axis=1, keepdims=True))
    return e[:, 1] / e.sum(axis=1) * 255.0


def normals255(v):
    """normals (utils.py:29-31): (F.normalize(x, p=2, dim=C) + 1) * 255 / 2, [B, H, W, 3]"""
    n = np.maximum(np.sqrt((v * v).sum(axis=1, keepdims=True)), 1e-12)
    return ((v / n + 1.0) * 255.0 / 2.0).transpose(0, 2, 3, 1)


def depth_clamped(v):
    """depth (utils.py:53-55): clamp(min=0)"""
    return np.maximum(v[:, 0], 0.0)


def depth_index(v):
    """visualization_utils.py:177-179 per image: (v - min) / (max - min) * 255, and which pixels are exact integers in any arithmetic
    (the zeros of the clamped map when the minimum is 0, the minimum and the maximum pixels).  A constant image: index 0 (the reference
    divides 0 by 0 there), all exact."""
    out, exact = np.zeros_like(v), np.zeros(v.shape, dtype=bool)
    for b in range(v.shape[0]):
        lo, hi = v[b].min(), v[b].max()
        if hi > lo:
            out[b] = (v[b] - lo) / (hi - lo) * 255.0
            exact[b] = (v[b] == lo) | (v[b] == hi)
        else:
            exact[b] = True
    return out, exact


def values(logits, task, size, rows=None, cols=None):
    """the fp64 map of `task` at `size` before truncation: (index, runner-up, gap) for the arg-max tasks, else the value array"""
    v = interpolate(logits, size, rows, cols)
    if task in ("semseg", "human_parts"):
        return top2(v)
    return {"edge": sigmoid255, "sal": softmax1_255, "normals": normals255, "depth": depth_clamped}[task](v)


def trunc8(v):
    """astype(np.uint8) on [0, 255] (visualization_utils.py:184, evaluate_utils.py:154)"""
    return np.floor(v).astype(np.uint8)


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------------
def labelcolormap(n):
    """visualization_utils.py:42-62"""
    i = np.arange(n)
    cmap = np.zeros((n, 3), dtype=np.uint8)
    for j in range(7):
        for k in range(3):
            cmap[:, k] ^= (((i >> (3 * j + k)) & 1) << (7 - j)).astype(np.uint8)
    return cmap


def cityscapes_colormap():
    """visualization_utils.py:14-39"""
    rows = "128 64 128 244 35 232 70 70 70 102 102 156 190 153 153 153 153 153 250 170 30 220 220 0 107 142 35 152 251 152 70 130 180 " \
           "220 20 60 255 0 0 0 0 142 0 0 70 0 60 100 0 80 100 0 0 230 119 11 32"
    cmap = np.zeros((256, 3), dtype=np.uint8)
    cmap[:19] = np.array(rows.split(), dtype=np.uint8).reshape(19, 3)
    return cmap


def semseg_colormap(db_name):
    """vis_semseg, visualization_utils.py:64-72"""
    return {"NYUD": labelcolormap(40), "PASCALContext": labelcolormap(21)}.get(db_name, cityscapes_colormap())


def label_ids():
    """get_cityscapes_class, utils.py:17-24"""
    t = np.arange(256, dtype=np.uint8)
    t[:19] = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]
    return t


def full_table(t):
    out = np.zeros((256, 3), dtype=np.uint8)
    out[:len(t)] = t
    return out


# ---- the save path: crop and skip (evaluate_utils.py:128-147) ---------------------------------------------------------------------------------
def crop_window(pred_size, img_size):
    (ph, pw), (ih, iw) = pred_size, img_size
    dh, dw = max(ph - ih, 0), max(pw - iw, 0)
    return dh // 2, dw // 2, ih, iw


def crop(arr, img_size):
    y0, x0, h, w = crop_window(arr.shape[:2], img_size)
    return arr[y0:y0 + h, x0:x0 + w]


def skipped(label, ignore_index):
    """evaluate_utils.py:129: the label map of the image holds nothing but ignore_index"""
    u = np.unique(label)
    return len(u) == 1 and u[0] == ignore_index


# ---- judging ----------------------------------------------------------------------------------------------------------------------------------------
def delta_of(deltas, task, identity):
    """the margin of `task` (tests/golden/render.json); 0 for an arg-max at identity size, where both sides hold the same fp32 logits"""
    return 0.0 if identity and task in ("semseg", "human_parts") else float(deltas[task])


def near_bytes(val, delta, exact=None):
    """the pixels a byte comparison leaves out: within delta of an integer without being one, and not known to be exact"""
    val = np.asarray(val, dtype=np.float64)
    near = (np.abs(val - np.rint(val)) < delta) & (val != np.rint(val))
    return near if exact is None else near & ~exact


def near_class(gap, delta):
    """the pixels an arg-max comparison leaves out: the two largest logits within delta of each other without being equal"""
    return (gap < delta) & (gap > 0)


def judge_bytes(got, val, delta, exact=None, lut=None):
    """got uint8 [...] (or [..., 3] colours of `lut`) against the fp64 values `val`.  Returns (share left out, mismatches outside the
    margin, left-out pixels that differ by more than one level)."""
    val = np.asarray(val, dtype=np.float64)
    near = near_bytes(val, delta, exact)
    want = np.clip(np.floor(val), 0, 255).astype(np.int64)
    lo, hi = np.clip(want - 1, 0, 255), np.clip(want + 1, 0, 255)
    if lut is None:
        same, loose = got == want, (got == want) | (got == lo) | (got == hi)
    else:
        eq = lambda i: (got == lut[i]).all(axis=-1)          # noqa: E731
        same, loose = eq(want), eq(want) | eq(lo) | eq(hi)
    return float(near.mean()), int((~same & ~near).sum()), int((~loose & near).sum())


def judge_class(got, idx, run, gap, delta, lut=None):
    """got uint8 class map (or its colours / label ids through `lut`) against (index, runner-up, gap)"""
    near = near_class(gap, delta)
    if lut is None:
        same, alt = got == idx, got == run
    elif lut.ndim == 1:
        same, alt = got == lut[idx], got == lut[run]
    else:
        same, alt = (got == lut[idx]).all(axis=-1), (got == lut[run]).all(axis=-1)
    return float(near.mean()), int((~same & ~near).sum()), int((~(same | alt) & near).sum())


def judge_vis(case, logits, got, deltas, depth_lut=None):
    """a case of tests/golden/render.json through the visualisation path: `got` uint8 [B, H, W] or [B, H, W, 3] in R, G, B order (for
    depth: the colours of `depth_lut`, or the index itself without one).  Constant depth images must hold index 0."""
    task, size = case["task"], case["size"]
    delta = delta_of(deltas, task, list(np.shape(logits)[2:]) == list(size))
    vals = values(logits, task, size)
    if task in ("semseg", "human_parts"):
        table = full_table(semseg_colormap(case["db"]) if task == "semseg" else labelcolormap(7))
        return judge_class(got, *vals, delta, lut=table)
    exact = None
    if task == "depth":
        vals, exact = depth_index(vals)
    return judge_bytes(got, vals, delta, exact=exact, lut=depth_lut if task == "depth" else None)


def judge_save(case, logits, got, deltas, i):
    """image i of a save-path case: `got` uint8 [h_i, w_i] (fp32 for depth, which must equal the clamped map)"""
    task = case["task"]
    h, w = np.shape(logits)[2:]
    y0, x0, hh, ww = crop_window((h, w), case["img_sizes"][i])
    vals = values(logits[i:i + 1], task, (h, w))
    cut = lambda a: a[0, y0:y0 + hh, x0:x0 + ww]             # noqa: E731
    if task in ("semseg", "human_parts"):
        return judge_class(got, *[cut(a) for a in vals], 0.0, lut=None if case.get("train_class", True) else label_ids())
    if task == "depth":
        return 0.0, int((got != cut(vals).astype(np.float32)).sum()), 0
    return judge_bytes(got, cut(vals), delta_of(deltas, task, True))


def near_vis(case, logits, deltas):
    """the left-out mask of judge_vis [B, H, W]"""
    task, size = case["task"], case["size"]
    delta = delta_of(deltas, task, list(np.shape(logits)[2:]) == list(size))
    vals = values(logits, task, size)
    if task in ("semseg", "human_parts"):
        return near_class(vals[2], delta)
    exact = None
    if task == "depth":
        vals, exact = depth_index(vals)
    near = near_bytes(vals, delta, exact)
    return near.any(axis=-1) if near.ndim == 4 else near
