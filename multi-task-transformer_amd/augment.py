"""Batch augmentation on the device: the reference's per-sample transform pipeline (TaskPrompter/utils/common_config.py:96-124 composing
data/transforms.py: RandomScaling, RandomCrop(cat_max_ratio), RandomHorizontalFlip, PhotoMetricDistortion, Normalize, PadImage,
AddIgnoreRegions, ToTensor) as three HIP entry points (csrc/augment.hip).

    aug = DeviceAugment(tasks, size)              # or: train, valid = DeviceAugment.from_config(p)
    params = aug.draw(shapes, rng)                # host: every random number of the batch -> AugParams, one row per sample
    batch = aug(samples, params)                  # device: [{'image': [H, W, 3] uint8 | fp32, task: [H, W, C] fp32}] -> {'image': [B, 3, h, w], ...}
    flat, shapes = aug.pack(samples)              # the two halves of the call: one packed buffer per key (torch.cat) ...
    batch = aug.run(flat, shapes, params)         # ... and the kernels, for a loader that delivers packed batches itself

The draws are the reference's, with one change of ORDER only: RandomCrop draws a crop location, tests it and draws again on failure, up to
10 times; `draw` takes all 11 locations up front (they are i.i.d.) and the select kernel picks the one the loop would have stopped at.
Preconditions: image values in [0, 255]; semseg / human_parts labels integral in [0, 255].  There is no CPU path: a CPU tensor raises."""
import random
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

CHANNELS = {"image": 3, "normals": 3}                                              # every other key has one channel
FILL = {"edge": 255.0, "human_parts": 255.0, "semseg": 255.0, "sal": 255.0, "depth": 0.0, "normals": 0.0}      # PadImage.fill_index
KIND = {"depth": _lib.AUG_DEPTH, "normals": _lib.AUG_NORMALS, "human_parts": _lib.AUG_HUMAN_PARTS}
N_CAND = _lib.AUG_CANDS
BRIGHTNESS_DELTA, CONTRAST_RANGE, SATURATION_RANGE, HUE_DELTA = 32, (0.5, 1.5), (0.5, 1.5), 18                    # PhotoMetricDistortion()


@dataclass
class AugParams:
    """One row per sample.  `scale` is the Python double the sizes were computed from; the kernels see it as fp32 (the value numpy uses
    when it divides a float32 array by a Python float), like beta and the alphas."""
    shapes: np.ndarray                        # int  [B, 2] source (H, W)
    scale: np.ndarray                         # fp64 [B]
    scaled: np.ndarray                        # int  [B, 2] (int(H * s), int(W * s)); the source size when not resized
    resized: np.ndarray                       # bool [B] s != 1.0
    cand_y: np.ndarray                        # int  [B, 11] crop offsets, candidates 0..9 tested and 10 the fall-back
    cand_x: np.ndarray
    n_test: np.ndarray                        # int  [B] 10 when the select kernel decides, 0 when candidate 0 is used as it is
    flip: np.ndarray                          # bool [B]
    bright: np.ndarray                        # bool [B], beta fp32 [B]
    beta: np.ndarray
    f_mode: np.ndarray                        # bool [B] contrast before saturation and hue
    contrast: np.ndarray                      # bool [B], c_alpha fp32 [B]
    c_alpha: np.ndarray
    sat: np.ndarray                           # bool [B], s_alpha fp32 [B]
    s_alpha: np.ndarray
    hue: np.ndarray                           # bool [B], hue_delta int [B] in [-18, 17]
    hue_delta: np.ndarray

    @classmethod
    def identity(cls, shapes):
        """no scaling, crop offset 0, no flip, no distortion: the valid-mode row"""
        shapes = np.asarray(shapes, dtype=np.int64).reshape(-1, 2)
        B = len(shapes)
        z, zb, zf = np.zeros(B, np.int64), np.zeros(B, bool), np.zeros(B, np.float32)
        return cls(shapes=shapes, scale=np.ones(B), scaled=shapes.copy(), resized=zb.copy(), cand_y=np.zeros((B, N_CAND), np.int64),
                   cand_x=np.zeros((B, N_CAND), np.int64), n_test=z.copy(), flip=zb.copy(), bright=zb.copy(), beta=zf.copy(), f_mode=zb.copy(),
                   contrast=zb.copy(), c_alpha=zf + 1, sat=zb.copy(), s_alpha=zf + 1, hue=zb.copy(), hue_delta=z.copy())

    def __len__(self):
        return len(self.shapes)

    def table(self):
        """int32 [B, MTT_AUG_COLS] of include/mtt_hip.h (floats as their bit patterns)"""
        L = _lib
        t = np.zeros((len(self), L.AUG_COLS), dtype=np.int32)
        f = t.view(np.float32)
        t[:, L.AUG_H], t[:, L.AUG_W] = self.shapes[:, 0], self.shapes[:, 1]
        t[:, L.AUG_SH], t[:, L.AUG_SW] = self.scaled[:, 0], self.scaled[:, 1]
        t[:, L.AUG_RESIZED], t[:, L.AUG_FLIP], t[:, L.AUG_NTEST] = self.resized, self.flip, self.n_test
        t[:, L.AUG_CHOSEN] = np.where(np.asarray(self.n_test) == N_CAND - 1, N_CAND - 1, 0)      # the select kernel lowers it to the first that passes
        t[:, L.AUG_CAND_Y:L.AUG_CAND_Y + N_CAND] = self.cand_y
        t[:, L.AUG_CAND_X:L.AUG_CAND_X + N_CAND] = self.cand_x
        t[:, L.AUG_BRIGHT], t[:, L.AUG_FMODE], t[:, L.AUG_CONTRAST], t[:, L.AUG_SAT], t[:, L.AUG_HUE] = self.bright, self.f_mode, self.contrast, self.sat, self.hue
        t[:, L.AUG_HDELTA] = self.hue_delta
        f[:, L.AUG_BETA], f[:, L.AUG_CALPHA], f[:, L.AUG_SALPHA] = self.beta, self.c_alpha, self.s_alpha
        f[:, L.AUG_SCALE] = np.asarray(self.scale, dtype=np.float64).astype(np.float32)
        return t


class DeviceAugment:
    def __init__(self, tasks, size, train=True, scale_factors=(0.5, 2.0), cat_max_ratio=0.75, flip_p=0.5, photometric=True,
                 mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), depth_ignore_to_minus1=True):
        self.tasks = list(tasks)
        self.size = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        self.train = bool(train)
        self.scale_factors = tuple(scale_factors)
        self.cat_max_ratio = float(cat_max_ratio)
        self.flip_p = float(flip_p)
        self.photometric = bool(photometric)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.depth_ignore_to_minus1 = bool(depth_ignore_to_minus1)
        unknown = [t for t in self.tasks if t not in FILL]
        if unknown:
            raise ValueError(f"no transform is defined for {unknown} (the reference's PadImage.fill_index has {sorted(FILL)})")
        if self.train and self.cat_max_ratio < 1.0 and "semseg" not in self.tasks:
            raise KeyError("semseg")          # RandomCrop(cat_max_ratio < 1) reads sample['semseg']: the reference fails there too
        self.rng = random.Random()

    @classmethod
    def from_config(cls, p):
        """(train, valid) as get_transformations(p) composes them; (None, None) for the data sets it has no transforms for"""
        if p["train_db_name"] not in ("NYUD", "PASCALContext"):
            return None, None
        tasks = list(p.TASKS.NAMES)
        return cls(tasks, p.TRAIN.SCALE, train=True), cls(tasks, p.TEST.SCALE, train=False)

    def __repr__(self):
        if not self.train:
            return f"DeviceAugment(Normalize, PadImage({self.size}), AddIgnoreRegions, ToTensor)"
        return (f"DeviceAugment(RandomScaling({self.scale_factors}), RandomCrop({self.size}, cat_max_ratio={self.cat_max_ratio}), "
                f"RandomHorizontalFlip({self.flip_p}), {'PhotoMetricDistortion, ' if self.photometric else ''}Normalize, PadImage({self.size}), "
                "AddIgnoreRegions, ToTensor)")

    # ---- host: the random numbers --------------------------------------------------------------------------------------------------------
    def draw(self, shapes, rng=None):
        rng = self.rng if rng is None else rng
        P = AugParams.identity(shapes)
        if not self.train:
            self._check_fits(P)
            return P
        h, w = self.size
        for i, (H, W) in enumerate(P.shapes.tolist()):
            s = rng.uniform(*self.scale_factors)                                   # RandomScaling.get_scale_factor
            P.scale[i] = s
            if s != 1.0:                                                           # RandomScaling.scale: int(x * scale) in Python doubles
                P.resized[i] = True
                P.scaled[i] = (int(H * s), int(W * s))
                if min(P.scaled[i]) < 1:
                    raise ValueError(f"sample {i}: {H}x{W} scaled by {s} is empty")
            Sh, Sw = P.scaled[i].tolist()
            if (Sh, Sw) != (h, w):                                                 # RandomCrop.get_random_crop_loc, 11 times
                for k in range(N_CAND):
                    P.cand_y[i, k] = rng.randint(0, max(Sh - h, 0))
                    P.cand_x[i, k] = rng.randint(0, max(Sw - w, 0))
                if self.cat_max_ratio < 1.0:
                    P.n_test[i] = N_CAND - 1
            P.flip[i] = rng.random() < self.flip_p                                 # RandomHorizontalFlip
            if self.photometric:                                                   # PhotoMetricDistortion.__call__
                P.bright[i] = rng.random() < 0.5
                if P.bright[i]:
                    P.beta[i] = rng.uniform(-BRIGHTNESS_DELTA, BRIGHTNESS_DELTA)
                P.f_mode[i] = rng.random() < 0.5
                if P.f_mode[i]:
                    self._contrast(P, i, rng)
                P.sat[i] = rng.random() < 0.5
                if P.sat[i]:
                    P.s_alpha[i] = rng.uniform(*SATURATION_RANGE)
                P.hue[i] = rng.random() < 0.5
                if P.hue[i]:
                    P.hue_delta[i] = rng.randint(-HUE_DELTA, HUE_DELTA - 1)
                if not P.f_mode[i]:
                    self._contrast(P, i, rng)
        return P

    @staticmethod
    def _contrast(P, i, rng):
        P.contrast[i] = rng.random() < 0.5
        if P.contrast[i]:
            P.c_alpha[i] = rng.uniform(*CONTRAST_RANGE)

    def _check_fits(self, P):
        h, w = self.size
        if (P.shapes[:, 0] > h).any() or (P.shapes[:, 1] > w).any():
            raise ValueError(f"valid mode pads to {self.size} and never crops: a sample larger than that has no place in a batch")

    # ---- device --------------------------------------------------------------------------------------------------------------------------
    def pack(self, samples):
        """the ragged batch as one flat device buffer per key (torch.cat of the flattened samples) and the samples' (H, W)"""
        keys = ["image"] + self.tasks
        if len(samples) == 0:
            raise ValueError("empty batch")
        for s in samples:
            for k in keys:
                t = s[k]
                if not t.is_cuda:
                    raise RuntimeError(f"DeviceAugment operates on HIP device memory only ('{k}' is on {t.device})")
                if t.dim() != 3 or t.shape[2] != CHANNELS.get(k, 1) or tuple(t.shape[:2]) != tuple(s["image"].shape[:2]):
                    raise ValueError(f"'{k}': expected [H, W, {CHANNELS.get(k, 1)}] with the image's H and W, got {tuple(t.shape)}")
                if t.dtype != samples[0][k].dtype or (t.dtype != torch.float32 and not (k == "image" and t.dtype == torch.uint8)):
                    raise TypeError(f"'{k}': {t.dtype} (image: uint8 or float32, labels: float32; one dtype per batch)")
        return {k: torch.cat([s[k].reshape(-1) for s in samples]) for k in keys}, [tuple(s["image"].shape[:2]) for s in samples]

    def __call__(self, samples, params=None):
        flat, shapes = self.pack(samples)
        return self.run(flat, shapes, params)

    def run(self, flat, shapes, params=None):
        """the kernels on a batch that `pack` (or a loader) has packed: flat[key] holds the samples' HWC elements back to back"""
        B = len(shapes)
        if params is None:
            params = self.draw(shapes)
        if len(params) != B or params.shapes.tolist() != [list(s) for s in shapes]:
            raise ValueError("params were drawn for other sample shapes")
        if not self.train:
            self._check_fits(params)
        dev = flat["image"].device
        h, w = self.size
        # the tables: pinned host copies (the entry points validate them) and their non-blocking uploads
        table_host = torch.empty((B, _lib.AUG_COLS), dtype=torch.int32, pin_memory=True)
        table_host.numpy()[...] = params.table()
        pixels = params.shapes[:, 0] * params.shapes[:, 1]
        start = np.concatenate([[0], np.cumsum(pixels)[:-1]]).astype(np.int64)
        off_host = torch.empty((2, B), dtype=torch.int64, pin_memory=True)       # row 0: one channel per pixel, row 1: three
        off_host.numpy()[0], off_host.numpy()[1] = start, 3 * start
        table, off = table_host.to(dev, non_blocking=True), off_host.to(dev, non_blocking=True)

        def packed(k):
            c = CHANNELS.get(k, 1)
            if not flat[k].is_cuda:
                raise RuntimeError(f"DeviceAugment operates on HIP device memory only ('{k}' is on {flat[k].device})")
            if flat[k].dtype != torch.float32 and not (k == "image" and flat[k].dtype == torch.uint8):
                raise TypeError(f"'{k}': {flat[k].dtype} (image: uint8 or float32, labels: float32)")
            return dict(src=flat[k], src_numel=flat[k].numel(), C=c, off=off[1 if c == 3 else 0], off_host=off_host[1 if c == 3 else 0],
                        table=table, table_host=table_host, B=B, h=h, w=w)

        def launch(name, **kw):
            rc = _lib.aug_call(name, **kw)
            if rc != 0:
                raise RuntimeError(f"mtt_{name}: the descriptor or its parameter table was refused (status {rc})")

        if (params.n_test != 0).any():
            launch("aug_select", cat_max_ratio=self.cat_max_ratio, **packed("semseg"))
        out = {"image": torch.empty((B, 3, h, w), dtype=torch.float32, device=dev)}
        launch("aug_image", out=out["image"], src_u8=int(flat["image"].dtype == torch.uint8), photometric=int(self.train and self.photometric),
            mean=self.mean, std=self.std, **packed("image"))
        for k in self.tasks:
            c = CHANNELS.get(k, 1)
            out[k] = torch.empty((B, c, h, w), dtype=torch.float32, device=dev)
            flags = torch.empty(B, dtype=torch.int32, device=dev) if k == "human_parts" else None
            launch("aug_labels", out=out[k], kind=KIND.get(k, _lib.AUG_PLAIN), fill=FILL[k], depth_ignore=int(self.depth_ignore_to_minus1), flags=flags,
                **packed(k))
        self.last_table = table                  # CHOSEN as the select kernel left it (read by the tests; a device tensor, no copy here)
        return out
