"""Predictions rendered and saved on the device: the stage of the reference that turns a batch of predictions into files,
vis_pred_for_one_task (TaskPrompter/utils/visualization_utils.py:80-199) and save_model_pred_for_one_task
(evaluation/evaluate_utils.py:68-154).  The reference interpolates the logits to the image size in fp32, applies get_output, copies the
int64 / fp32 map to the host and colours it there; here one HIP kernel (csrc/render.hip) reads the logits once and writes the 1 or 3
bytes per pixel that the file needs, and only those bytes reach the host.

    r = PredictionRenderer("Cityscapes3D")                # or PredictionRenderer.from_config(p)
    rgb = r.render(output["semseg"], "semseg", (1024, 2048))          # uint8 [B, H, W, 3] on the device
    maps = r.raw(output["edge"], "edge", img_sizes)                   # what the save path writes: per image uint8 [h_i, w_i], fp32 for depth
    vis_pred_for_one_task(p, sample, output, save_dir, task)          # the reference's signatures: one device-to-host copy per task and
    save_model_pred_for_one_task(p, batch_idx, sample, output, save_dirs, task, epoch)      # batch, PNG / .mat encoding on host threads

Neither `render` nor `raw` synchronises with the host; tables and workspaces are allocated on first use, so after one warm-up call a
batch can be captured in a hipGraph.  There is no CPU path: a CPU tensor or logits other than fp32 raise RuntimeError.

Differences from the reference, all deliberate:
  * depth colours: the reference calls cv2.applyColorMap(.., COLORMAP_JET).  The default `depth_lut` is matplotlib's `jet` sampled at 256
    points (JET below), which is NOT OpenCV's table; pass OpenCV's own, in R, G, B order, for byte equality with cv2.applyColorMap.
  * a depth map that is constant over an image gets colour index 0 everywhere; the reference divides 0 by 0 there.
  * the save path's bare `raise` for a 3-D prediction (evaluate_utils.py:148-149) is a RuntimeError that names the task.  get_output
    leaves depth as [B, H, W, 1], so the reference's save path raises for depth as well and never reaches its own savemat branch; here
    the [H, W] map is written, which is what that branch is for.
  * task '3ddet' (bbox2json / bbox2fig: host JSON and drawing) raises NotImplementedError.
  * get_output clamps the caller's depth prediction in place (output.clamp_); here the prediction is left as it is."""
import os
from collections.abc import Mapping
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib

CS_VALID_CLASSES = (7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33)      # utils/utils.py:18
CLASS_TASKS = ("semseg", "human_parts")
TASKS = CLASS_TASKS + ("sal", "edge", "normals", "depth")

# matplotlib 3.10's colormaps["jet"](np.arange(256), bytes=True)[:, :3], R, G, B: committed so that matplotlib is not needed at run time
JET = np.frombuffer(bytes.fromhex(
    "00007f00008400008800008d00009100009600009a00009f0000a30000a80000ac0000b10000b60000ba0000bf0000c3"
    "0000c80000cc0000d10000d50000da0000de0000e30000e80000ec0000f10000f50000fa0000fe0000ff0000ff0000ff"
    "0000ff0004ff0008ff000cff0010ff0014ff0018ff001cff0020ff0024ff0028ff002cff0030ff0034ff0038ff003cff"
    "0040ff0044ff0048ff004cff0050ff0054ff0058ff005cff0060ff0064ff0068ff006cff0070ff0074ff0078ff007cff"
    "0080ff0084ff0088ff008cff0090ff0094ff0098ff009cff00a0ff00a4ff00a8ff00acff00b0ff00b4ff00b8ff00bcff"
    "00c0ff00c4ff00c8ff00ccff00d0ff00d4ff00d8ff00dcfe00e0fa00e4f702e8f405ecf108f0ed0cf4ea0ff8e712fce4"
    "15ffe118ffdd1cffda1fffd722ffd425ffd029ffcd2cffca2fffc732ffc336ffc039ffbd3cffba3fffb742ffb346ffb0"
    "49ffad4cffaa4fffa653ffa356ffa059ff9d5cff9a5fff9663ff9366ff9069ff8d6cff8970ff8673ff8376ff8079ff7d"
    "7cff7980ff7683ff7386ff7089ff6c8dff6990ff6693ff6396ff5f9aff5c9dff59a0ff56a3ff53a6ff4faaff4cadff49"
    "b0ff46b3ff42b7ff3fbaff3cbdff39c0ff36c3ff32c7ff2fcaff2ccdff29d0ff25d4ff22d7ff1fdaff1cddff18e0ff15"
    "e4ff12e7ff0feaff0cedff08f1fc05f4f802f7f400faf000feed00ffe900ffe500ffe200ffde00ffda00ffd700ffd300"
    "ffcf00ffcb00ffc800ffc400ffc000ffbd00ffb900ffb500ffb100ffae00ffaa00ffa600ffa300ff9f00ff9b00ff9800"
    "ff9400ff9000ff8c00ff8900ff8500ff8100ff7e00ff7a00ff7600ff7300ff6f00ff6b00ff6700ff6400ff6000ff5c00"
    "ff5900ff5500ff5100ff4d00ff4a00ff4600ff4200ff3f00ff3b00ff3700ff3400ff3000ff2c00ff2800ff2500ff2100"
    "ff1d00ff1a00ff1600fe1200fa0f00f50b00f10700ec0300e80000e30000de0000da0000d50000d10000cc0000c80000"
    "c30000bf0000ba0000b60000b10000ac0000a80000a300009f00009a00009600009100008d00008800008400007f0000"
), dtype=np.uint8).reshape(256, 3)


def cityscapes_colormap():
    """create_cityscapes_label_colormap (visualization_utils.py:14-39): 256 rows, the 19 train classes coloured, the rest black"""
    cmap = np.zeros((256, 3), dtype=np.uint8)
    cmap[:19] = [(128, 64, 128), (244, 35, 232), (70, 70, 70), (102, 102, 156), (190, 153, 153), (153, 153, 153), (250, 170, 30),
                 (220, 220, 0), (107, 142, 35), (152, 251, 152), (70, 130, 180), (220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70),
                 (0, 60, 100), (0, 80, 100), (0, 0, 230), (119, 11, 32)]
    return cmap


def labelcolormap(n):
    """labelcolormap (visualization_utils.py:46-62): bit k of the class index, three bits at a time, goes to bit 7 - j of r / g / b"""
    cmap = np.zeros((n, 3), dtype=np.uint8)
    for i in range(n):
        rgb, idx = [0, 0, 0], i
        for j in range(7):
            for k in range(3):
                rgb[k] ^= ((idx >> k) & 1) << (7 - j)
            idx >>= 3
        cmap[i] = rgb
    return cmap


def semseg_colormap(db_name):
    """vis_semseg (visualization_utils.py:64-72)"""
    if db_name == "NYUD":
        return labelcolormap(40)
    if db_name == "PASCALContext":
        return labelcolormap(21)
    return cityscapes_colormap()


def cityscapes_label_ids():
    """get_cityscapes_class (utils/utils.py:17-24) as a table: train class 0..18 -> its label id, every other value kept"""
    table = np.arange(256, dtype=np.uint8)
    table[:19] = CS_VALID_CLASSES
    return table


def crop_window(pred_size, img_size):
    """(y0, x0, h, w): the centre crop of a padded prediction (evaluate_utils.py:133-147)"""
    (ph, pw), (ih, iw) = pred_size, (int(img_size[0]), int(img_size[1]))
    if ih < 1 or iw < 1 or ih > ph or iw > pw:
        raise ValueError(f"img_size {(ih, iw)} does not fit the prediction {(ph, pw)} (the reference's assert, evaluate_utils.py:147)")
    return ((ph - ih) // 2, (pw - iw) // 2, ih, iw)


def _sizes(img_size, count):
    """meta['img_size'] as the default collate delivers it (a [B, 2] tensor or array, or a list of pairs) -> host ints"""
    rows = img_size.tolist() if hasattr(img_size, "tolist") else list(img_size)
    out = [(int(r[0]), int(r[1])) for r in rows]
    if len(out) != count:
        raise ValueError(f"meta['img_size'] holds {len(out)} sizes for a batch of {count}")
    return out


class PredictionRenderer:
    def __init__(self, db_name, depth_lut=None, bgr=False):
        self.db_name = str(db_name)
        self.bgr = bool(bgr)
        lut = JET if depth_lut is None else np.asarray(depth_lut)
        if lut.shape != (256, 3) or lut.dtype != np.uint8:
            raise ValueError(f"depth_lut: expected uint8 [256, 3] in R, G, B order, got {lut.dtype} {lut.shape}")
        self.tables = {"semseg": semseg_colormap(self.db_name), "human_parts": labelcolormap(7), "depth": np.array(lut),
                       "label_ids": cityscapes_label_ids()}
        self._device = {}                                   # (what, device, ...) -> uploaded table / workspace

    @classmethod
    def from_config(cls, p):
        return cls(p["train_db_name"])

    def __repr__(self):
        return f"PredictionRenderer({self.db_name!r}, {'BGR' if self.bgr else 'RGB'})"

    # ---- tables and workspaces, uploaded on first use ---------------------------------------------------------------------------------
    def _table(self, name, dev):
        key = ("table", name, str(dev))
        if key not in self._device:
            t = self.tables[name]
            if t.ndim == 2:
                full = np.zeros((256, 3), dtype=np.uint8)
                full[:len(t)] = t[:, ::-1] if self.bgr else t
                t = full
            self._device[key] = torch.from_numpy(np.ascontiguousarray(t)).to(dev)
        return self._device[key]

    def _minmax(self, batch, dev):
        key = ("minmax", batch, str(dev))
        if key not in self._device:
            self._device[key] = torch.zeros(2, batch, dtype=torch.int32, device=dev)
        return self._device[key]

    def _windows(self, rows, dev):
        key = ("win", tuple(rows), str(dev))
        if key not in self._device:
            host = torch.tensor(rows, dtype=torch.int64).reshape(len(rows), 5)
            self._device[key] = (host, host.to(dev))
        return self._device[key]

    # ---- the launches -----------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check(logits, task):
        if task == "3ddet":
            raise NotImplementedError("task '3ddet' (bbox2json / bbox2fig) is not rendered on the device")
        if task not in TASKS:
            raise ValueError(f"task {task!r}: select one of {TASKS}")
        if not isinstance(logits, torch.Tensor) or not logits.is_cuda:
            raise RuntimeError(f"PredictionRenderer operates on HIP device memory only ('{task}' is on "
                               f"{logits.device if isinstance(logits, torch.Tensor) else type(logits).__name__})")
        if logits.dtype != torch.float32:
            raise RuntimeError(f"'{task}': fp32 logits as the model wrappers return them, got {logits.dtype}")
        if logits.dim() != 4 or not logits.is_contiguous():
            raise ValueError(f"'{task}': expected contiguous NCHW logits, got shape {tuple(logits.shape)} strides {logits.stride()}")
        want = {"sal": 2, "edge": 1, "normals": 3, "depth": 1}.get(task)
        if want is not None and logits.shape[1] != want:
            raise ValueError(f"'{task}': expected {want} channel(s), got {logits.shape[1]}")

    def _out(self, out, numel, dtype, dev):
        if out is None:
            return torch.empty(numel, dtype=dtype, device=dev)
        if out.dtype != dtype or out.numel() != numel or out.device != dev or not out.is_contiguous():
            raise ValueError(f"out: expected contiguous {dtype} with {numel} elements on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        return out.view(-1)

    def _map(self, logits, task, size, out_kind, table, out, out_pixels, win=None, stats=None):
        B, C, h, w = logits.shape
        mode = {"semseg": _lib.RENDER_CLASS, "human_parts": _lib.RENDER_CLASS, "sal": _lib.RENDER_SOFTMAX1_255, "edge": _lib.RENDER_SIGMOID255,
                "normals": _lib.RENDER_NORMALS, "depth": _lib.RENDER_DEPTH}[task]
        kw = dict(src=logits, B=B, C=C, h=h, w=w, H=size[0], W=size[1])
        if win is not None:
            kw.update(win_host=win[0], win=win[1])
        if stats is not None:
            self._launch("render_minmax", minmax=stats, **kw)
        self._launch("render_map", out=out, out_pixels=out_pixels, table=table, minmax=stats, mode=mode, out_kind=out_kind,
                     swap_rb=int(self.bgr), **kw)

    @staticmethod
    def _launch(name, **kw):
        rc = _lib.render_call(name, **kw)
        if rc != 0:
            raise RuntimeError(f"mtt_{name}: the descriptor was refused (status {rc})")

    def render(self, output_task, task, size, out=None):
        """uint8 [B, H, W] (sal, edge) or [B, H, W, 3] on the device: the array vis_pred_for_one_task hands to its file writer, channels in
        R, G, B order (B, G, R with bgr=True, the reference's in-memory order).  `out`: a contiguous uint8 tensor of that many elements."""
        self._check(output_task, task)
        B, C = output_task.shape[:2]
        H, W = int(size[0]), int(size[1])
        dev = output_task.device
        table, stats, channels = None, None, 3
        if task in CLASS_TASKS:
            if C > len(self.tables[task]):
                raise ValueError(f"'{task}': {C} classes, the colour map of {self.db_name} has {len(self.tables[task])}")
            kind, table = _lib.RENDER_OUT_LUT3, self._table(task, dev)
        elif task == "depth":
            kind, table, stats = _lib.RENDER_OUT_LUT3, self._table("depth", dev), self._minmax(B, dev)
        elif task == "normals":
            kind = _lib.RENDER_OUT_RGB3
        else:
            kind, channels = _lib.RENDER_OUT_U8, 1
        flat = self._out(out, B * H * W * channels, torch.uint8, dev)
        self._map(output_task, task, (H, W), kind, table, flat, B * H * W, stats=stats)
        return flat.view(B, H, W, 3) if channels == 3 else flat.view(B, H, W)

    def raw_layout(self, pred_size, img_sizes):
        """the packed output of `raw`: per image (y0, x0, h, w, offset in pixels), every offset a multiple of 4, and the total"""
        rows, off = [], 0
        for s in img_sizes:
            y0, x0, h, w = crop_window(pred_size, s)
            rows.append((y0, x0, h, w, off))
            off += (h * w + 3) & ~3
        return rows, off

    def raw(self, output_task, task, img_sizes, semseg_save_train_class=True, out=None):
        """what save_model_pred_for_one_task writes, per image: uint8 [h_i, w_i] (the class index, Cityscapes label ids with
        semseg_save_train_class=False, the truncated edge / saliency value) or fp32 for depth, centre-cropped to img_sizes[i].  The maps
        are views of one packed buffer (`out`, when given: contiguous, raw_layout's total elements of uint8 / fp32)."""
        self._check(output_task, task)
        if task == "normals":
            raise RuntimeError("task 'normals': a 3-D prediction is not saved by save_model_pred_for_one_task (evaluate_utils.py:148-149)")
        B, C, h, w = output_task.shape
        dev = output_task.device
        sizes = list(img_sizes)
        if len(sizes) != B:
            raise ValueError(f"{len(sizes)} image sizes for a batch of {B}")
        rows, total = self.raw_layout((h, w), sizes)
        kind, table, dtype = _lib.RENDER_OUT_U8, None, torch.uint8
        if task == "depth":
            kind, dtype = _lib.RENDER_OUT_F32, torch.float32
        elif task == "semseg" and not semseg_save_train_class:
            kind, table = _lib.RENDER_OUT_LUT1, self._table("label_ids", dev)
        if task in CLASS_TASKS and C > 256:
            raise ValueError(f"'{task}': {C} classes do not fit a byte")
        flat = self._out(out, total, dtype, dev)
        self._map(output_task, task, (h, w), kind, table, flat, total, win=self._windows(rows, dev))
        return [flat[o:o + hh * ww].view(hh, ww) for (_, _, hh, ww, o) in rows]


_RENDERERS = {}


def _renderer(p):
    db = p["train_db_name"]
    if db not in _RENDERERS:
        _RENDERERS[db] = PredictionRenderer(db)
    return _RENDERERS[db]


def _write_all(jobs):
    """encode in a thread pool, as the reference does (visualization_utils.py:193-196)"""
    if jobs:
        with ThreadPoolExecutor() as ex:
            for f in [ex.submit(fn, *args) for fn, *args in jobs]:
                f.result()


def _save_png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def _save_mat(path, arr):
    import scipy.io as sio
    sio.savemat(path, {"depth": arr})


@torch.no_grad()
def vis_pred_for_one_task(p, sample, output, save_dir, task):
    """{save_dir}/{img_name}_{task}.png per image, in R, G, B order: the colours cv2.imwrite shows for the reference's B, G, R array"""
    if task == "3ddet":
        raise NotImplementedError("task '3ddet' (bbox2fig) is not rendered on the device")
    meta = sample["meta"]
    size = meta["img_size"][0]                              # the reference assumes one size per batch (:122-124)
    arr = _renderer(p).render(output[task], task, (int(size[0]), int(size[1]))).cpu().numpy()
    names = meta["img_name"]
    _write_all([(_save_png, os.path.join(save_dir, "{}_{}.png".format(names[i], task)), arr[i]) for i in range(arr.shape[0])])


@torch.no_grad()
def save_model_pred_for_one_task(p, batch_idx, sample, output, save_dirs, task=None, epoch=None):
    """{save_dirs[task]}/{img_name}.png (.mat for depth) per image whose label map is not all ignore_index.  TaskPrompter's signature;
    InvPT's call (p, sample, output, save_dirs, task, epoch=epoch) is recognised by the sample in second place."""
    if isinstance(batch_idx, Mapping):
        sample, output, save_dirs, task = batch_idx, sample, output, save_dirs
    if task == "3ddet":
        raise NotImplementedError("task '3ddet' (bbox2json / bbox2fig) is not saved on the device")
    if task == "normals":
        raise RuntimeError("task 'normals': a 3-D prediction is not saved by save_model_pred_for_one_task (evaluate_utils.py:148-149)")
    meta, logits = sample["meta"], output[task]
    r = _renderer(p)
    r._check(logits, task)
    B, _, h, w = logits.shape
    train_class = bool(p.get("semseg_save_train_class", True)) or p["train_db_name"] != "Cityscapes3D"
    rows, total = r.raw_layout((h, w), _sizes(meta["img_size"], B))
    item = 4 if task == "depth" else 1
    # the rendered maps and the per-image "label is all ignore_index" flags (:129-130) share one buffer and one device-to-host copy
    buf = torch.empty(total * item + B, dtype=torch.uint8, device=logits.device)
    body = buf[:total * item]
    r.raw(logits, task, [(hh, ww) for (_, _, hh, ww, _) in rows], semseg_save_train_class=train_class,
          out=body.view(torch.float32) if item == 4 else body)
    label = sample[task]
    skip = (label.reshape(B, -1) == p["ignore_index"]).all(dim=1)
    buf[total * item:].copy_(skip.to(device=logits.device, dtype=torch.uint8))
    host = buf.cpu().numpy()
    flags = host[total * item:]
    maps = host[:total * item].view(np.float32) if item == 4 else host[:total * item]
    jobs = []
    for i, (_, _, hh, ww, off) in enumerate(rows):
        if flags[i]:
            continue
        arr = maps[off:off + hh * ww].reshape(hh, ww)
        stem = os.path.join(save_dirs[task], meta["img_name"][i])
        jobs.append((_save_mat, stem + ".mat", arr) if task == "depth" else (_save_png, stem + ".png", arr))
    _write_all(jobs)


@torch.no_grad()
def save_model_pred_for_one_task_invpt(p, sample, output, save_dirs, task=None, epoch=None):
    """InvPT's signature (InvPT/evaluation/evaluate_utils.py:69)"""
    return save_model_pred_for_one_task(p, 0, sample, output, save_dirs, task=task, epoch=epoch)
