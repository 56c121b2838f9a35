"""Cityscapes-3D batches prepared on the device: the per-sample work of the reference's dataset class
(TaskPrompter/data/cityscapes3d.py:137-241: BGR -> RGB, Pillow's bilinear resize of the image, encode_segmap, the disparity decoding with
its sky mask, Pillow's nearest resize of both label maps, ToTensor + Normalize) as two HIP entry points (csrc/cs3d.hip).

    prep = Cityscapes3DPrepare(tasks, img_size, dd_label_map_size)      # or: train, valid = Cityscapes3DPrepare.from_config(p)
    batch = prep(samples)             # [{'image': [H, W, 3] uint8, 'semseg': [H, W] uint8 labelIds, 'depth': [H, W] uint16 disparity, ...}]
    packed = prep.pack(samples)       # the two halves of the call: the stacked sources ...
    batch = prep.run(packed)          # ... and the kernels, for a loader that delivers stacked batches itself
    prep.check(batch)                 # the reference's ValueError for class values outside 0..18 / 255; the ONE synchronising call

`samples` are the decoded files as they are (cv2.imread's BGR order unless bgr=False); PNG / JSON decoding and load_det stay on the host,
and every key other than image / semseg / depth is handed through.  The frames of a batch have one size.  The resampling tables are
Pillow's, built here in Python doubles and uploaded once per (in, out) pair.  There is no CPU path: a CPU tensor raises."""
import math

import numpy as np
import torch

from . import _lib

PRECISION_BITS = 22                     # Pillow's Resample.c: 32 - 8 - 2
ORI_IMG_SIZE = (1024, 2048)             # cityscapes3d.py:102, a constant of the reference
INVALID_MESSAGE = "Segmentation map contained invalid class values"


def bilinear_tables(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter along one axis: (bounds int32 [n_out, 2] holding the
    first source index and the tap count, coeff int32 [n_out, ksize]).  Equal sizes: the identity (one tap of weight 2^22), which is what
    skipping the axis computes."""
    if n_in == n_out:
        idx = np.arange(n_out, dtype=np.int32)
        return np.stack([idx, np.ones_like(idx)], axis=1), np.full((n_out, 1), 1 << PRECISION_BITS, dtype=np.int32)
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coeff = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            v = abs((x + xmin - center + 0.5) * ss)
            v = 1.0 - v if v < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            coeff[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, coeff


def nearest_table(n_in, n_out):
    """Pillow's ImagingScaleAffine along one axis: the source index (int)xo, xo starting at half a step and ADVANCED BY ADDITION (a product
    (x + 0.5) * in / out rounds differently and lands on other pixels)."""
    step = n_in / n_out
    xo = 0.0 + step * 0.5
    idx = np.zeros(n_out, dtype=np.int32)
    for x in range(n_out):
        xin = int(xo)
        if not 0 <= xin < n_in:
            raise ValueError(f"nearest {n_in} -> {n_out}: index {xin} at {x}")
        idx[x] = xin
        xo += step
    return idx


class InvalidSegmentation(ValueError):
    """the reference's ValueError, with the batch indices of the images that raised it in `images`"""

    def __init__(self, images):
        super().__init__(f"{INVALID_MESSAGE} (images {images} of the batch)")
        self.images = images


class Cityscapes3DPrepare:
    def __init__(self, tasks, img_size, dd_label_map_size, ori_img_size=ORI_IMG_SIZE, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                 bgr=True):
        self.tasks = list(tasks)
        self.img_size = (int(img_size[0]), int(img_size[1]))
        self.dd_label_map_size = (int(dd_label_map_size[0]), int(dd_label_map_size[1]))
        self.ori_img_size = (int(ori_img_size[0]), int(ori_img_size[1]))
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.bgr = bool(bgr)
        if "depth" in self.tasks and "semseg" not in self.tasks:
            # the reference reads `lbl` for the sky mask and fails with a NameError when semseg was not loaded
            raise ValueError("'depth' needs 'semseg' among the tasks: the sky mask of the disparity map is read from the label ids")
        if min(self.img_size + self.dd_label_map_size) < 1:
            raise ValueError(f"empty output size {self.img_size} / {self.dd_label_map_size}")
        self._tables = {}                                   # (kind, in, out, device) -> uploaded tables

    @classmethod
    def from_config(cls, p):
        """(train, valid) as get_train_dataset / get_val_dataset construct CITYSCAPES3D (common_config.py:150-153, 189-192); (None, None)
        for the data sets whose samples go through data/transforms.py (DeviceAugment.from_config)"""
        if p["train_db_name"] != "Cityscapes3D":
            return None, None
        tasks = list(p.TASKS.NAMES)
        test = p.TEST.SCALE if "TEST" in p else p.TRAIN.SCALE
        return cls(tasks, p.TRAIN.SCALE, p.dd_label_map_size), cls(tasks, test, p.dd_label_map_size)

    def __repr__(self):
        return (f"Cityscapes3DPrepare({self.tasks}, img_size={self.img_size}, dd_label_map_size={self.dd_label_map_size}, "
                f"{'BGR' if self.bgr else 'RGB'} sources)")

    # ---- host: sizes and tables -----------------------------------------------------------------------------------------------------------
    def label_size(self, src_size):
        """the label maps are resampled when dd_label_map_size differs from the CONSTANT ori_img_size, not from the frame (:210, :216)"""
        return tuple(src_size) if self.dd_label_map_size == self.ori_img_size else self.dd_label_map_size

    def image_tables(self, src_size):
        """per axis (bounds, coeff), y then x; None when the image keeps its size (Pillow returns a copy)"""
        if tuple(src_size) == self.img_size:
            return None
        return bilinear_tables(src_size[0], self.img_size[0]), bilinear_tables(src_size[1], self.img_size[1])

    def label_tables(self, src_size):
        """(yin, xin); None when no resize applies"""
        if self.dd_label_map_size == self.ori_img_size:
            return None
        return nearest_table(src_size[0], self.dd_label_map_size[0]), nearest_table(src_size[1], self.dd_label_map_size[1])

    def _uploaded(self, kind, src_size, dev):
        key = (kind, tuple(src_size), str(dev))
        if key not in self._tables:
            tabs = self.image_tables(src_size) if kind == "image" else self.label_tables(src_size)
            if tabs is None:
                self._tables[key] = None
            else:
                flat = [a for t in tabs for a in (t if isinstance(t, tuple) else (t,))]
                host = [torch.from_numpy(np.ascontiguousarray(a)) for a in flat]
                self._tables[key] = (host, [t.to(dev) for t in host])
        return self._tables[key]

    # ---- device ---------------------------------------------------------------------------------------------------------------------------
    def pack(self, samples):
        """the batch as one stacked device tensor per source ('image' [B, H, W, 3], 'semseg' / 'depth' [B, H, W]) plus what is handed through"""
        if len(samples) == 0:
            raise ValueError("empty batch")
        keys = ["image"] + [t for t in ("semseg", "depth") if t in self.tasks]
        want = {"image": (torch.uint8,), "semseg": (torch.uint8,), "depth": (torch.uint16, torch.int16)}
        H, W = samples[0]["image"].shape[:2]
        for s in samples:
            for k in keys:
                if k not in s:
                    raise KeyError(k)
                t = s[k]
                if not t.is_cuda:
                    raise RuntimeError(f"Cityscapes3DPrepare operates on HIP device memory only ('{k}' is on {t.device})")
                if tuple(t.shape) != ((H, W, 3) if k == "image" else (H, W)):
                    raise ValueError(f"'{k}': expected {(H, W, 3) if k == 'image' else (H, W)} (one frame size per batch), got {tuple(t.shape)}")
                if t.dtype not in want[k]:
                    raise TypeError(f"'{k}': {t.dtype} (the decoded file: image and labelIds uint8, disparity uint16)")
        packed = {k: torch.stack([s[k] for s in samples]) for k in keys}
        packed["meta"] = [dict(s.get("meta", {})) for s in samples]
        packed["other"] = [{k: v for k, v in s.items() if k not in keys and k != "meta"} for s in samples]
        return packed

    def __call__(self, samples):
        return self.run(self.pack(samples))

    def run(self, packed, out=None):
        """the kernels on a stacked batch.  `out` may hold preallocated contiguous tensors for 'image', 'semseg', 'depth' and 'flags'"""
        given = dict(out or {})

        def alloc(key, shape, dtype):
            t = given.get(key)
            if t is None:
                return torch.empty(shape, dtype=dtype, device=dev)
            if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                raise ValueError(f"out['{key}']: expected contiguous {dtype} {tuple(shape)} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
            return t

        img = packed["image"]
        for k in ("image", "semseg", "depth"):
            if k in packed and not packed[k].is_cuda:
                raise RuntimeError(f"Cityscapes3DPrepare operates on HIP device memory only ('{k}' is on {packed[k].device})")
        if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8 or not img.is_contiguous():
            raise ValueError(f"'image': expected contiguous uint8 [B, H, W, 3], got {img.dtype} {tuple(img.shape)}")
        B, H, W = img.shape[:3]
        dev = img.device
        h, w = self.img_size
        out = {"image": alloc("image", (B, 3, h, w), torch.float32)}
        tabs = self._uploaded("image", (H, W), dev)
        kw = {}
        if tabs is not None:
            (yb_h, yc_h, xb_h, xc_h), (yb, yc, xb, xc) = tabs
            kw = dict(xtab=xb, ytab=yb, xtab_host=xb_h, ytab_host=yb_h, xcoeff=xc, ycoeff=yc, xn=w, yn=h, xk=xc.shape[1], yk=yc.shape[1])
        self._launch("cs3d_image", src=img, out=out["image"], B=B, H=H, W=W, h=h, w=w, bgr=int(self.bgr), mean=self.mean, std=self.std, **kw)
        if "semseg" in self.tasks:
            lab = packed["semseg"]
            if tuple(lab.shape) != (B, H, W) or lab.dtype != torch.uint8 or not lab.is_contiguous():
                raise ValueError(f"'semseg': expected contiguous uint8 {(B, H, W)}, got {lab.dtype} {tuple(lab.shape)}")
            disp = packed["depth"] if "depth" in self.tasks else None
            if disp is not None and (tuple(disp.shape) != (B, H, W) or disp.dtype not in (torch.uint16, torch.int16) or not disp.is_contiguous()):
                raise ValueError(f"'depth': expected contiguous uint16 {(B, H, W)}, got {disp.dtype} {tuple(disp.shape)}")
            lh, lw = self.label_size((H, W))
            out["semseg"] = alloc("semseg", (B, lh, lw), torch.int64)
            out["flags"] = alloc("flags", (B,), torch.int32)
            if disp is not None:
                out["depth"] = alloc("depth", (B, 1, lh, lw), torch.float32)
            tabs = self._uploaded("labels", (H, W), dev)
            kw = {}
            if tabs is not None:
                (yin_h, xin_h), (yin, xin) = tabs
                kw = dict(xtab=xin, ytab=yin, xtab_host=xin_h, ytab_host=yin_h, xn=lw, yn=lh)
            self._launch("cs3d_labels", src=lab, disp=disp, out=out.get("depth"), semseg=out["semseg"], flags=out["flags"], B=B, H=H, W=W, h=lh, w=lw,
                         **kw)
        # meta, in xy order as cityscapes3d.py:140-144
        out["meta"] = [dict(m, img_size=(H, W), dd_label_map_size=self.dd_label_map_size, scale_factor=np.array([w / W, h / H]))
                       for m in packed.get("meta", [{} for _ in range(B)])]
        for k in sorted({k for o in packed.get("other", []) for k in o}):
            out[k] = [o.get(k) for o in packed["other"]]
        return out

    @staticmethod
    def _launch(name, **kw):
        rc = _lib.cs3d_call(name, **kw)
        if rc != 0:
            raise RuntimeError(f"mtt_{name}: the descriptor was refused (status {rc})")

    @staticmethod
    def check(batch):
        """reads the validity flags (a device-to-host copy: this synchronises) and raises as cityscapes3d.py:224-226 does"""
        if "flags" not in batch:
            return
        bad = [i for i, f in enumerate(batch["flags"].cpu().tolist()) if f != 0]
        if bad:
            raise InvalidSegmentation(bad)
