"""Host side of the 3ddet inference post-processing on the HIP kernels of csrc/det_decode.hip (ABI 16): the descriptor geometry, the
caller-owned buffers and the four launches select -> decode -> segmented NMS -> collect.  Nothing here reads the device: the candidate
count per image follows from the level shapes and nms_pre, every buffer has a fixed capacity, and the kept counts stay in device memory
until the caller copies `out` (rows and counts in ONE allocation, so one device-to-host copy fetches both).  DetModel.get_bboxes /
get_results_from_bbox (det_model.py) are the public interface."""
import torch

from . import _lib, ops

MAX_LEVELS = 8
MAX_CAND, MAX_CLASSES, OUT_COLS = _lib.DET_MAX_CAND, _lib.DET_MAX_CLASSES, _lib.DET_OUT_COLS


class DecodeLimitError(NotImplementedError):
    """more candidates per image or more classes than the decode kernels take"""


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def geometry(sizes, strides, nms_pre, denorm):
    """level shapes -> the descriptor's per-level constants and offsets.  `denorm`: the maps are the head's stride-normalised ones
    (the kernel multiplies offsets and 2-D distances by the stride) or already denormalised (multiplier 1)."""
    L = len(sizes)
    if not 0 < L <= MAX_LEVELS or L != len(strides):
        raise ValueError(f"{L} feature levels for {len(strides)} strides (1..{MAX_LEVELS} levels)")
    pad = lambda v, n, z: list(v) + [z] * (n - len(v))
    H, W = [int(h) for h, _ in sizes], [int(w) for _, w in sizes]
    cand, key = [0], [0]
    for h, w in zip(H, W):
        P = h * w
        cand.append(cand[-1] + (nms_pre if 0 < nms_pre < P else P))
        key.append(key[-1] + P)
    return dict(H=pad(H, 8, 0), W=pad(W, 8, 0), stride=pad([_f32(s) for s in strides], 8, 0.0),
                half=pad([_f32(s // 2) for s in strides], 8, 0.0), denorm=pad([_f32(s) if denorm else 1.0 for s in strides], 8, 0.0),
                cand_off=pad(cand, 9, cand[-1]), key_off=pad(key, 9, key[-1]), nlev=L, N=cand[-1], nms_pre=int(nms_pre))


def check_limits(N, C):
    if N > MAX_CAND:
        raise DecodeLimitError(f"{N} candidates per image (the decode kernels take up to {MAX_CAND}: lower nms_pre)")
    if C > MAX_CLASSES:
        raise DecodeLimitError(f"{C} classes (the decode kernels take up to {MAX_CLASSES})")


def nms_buffers(B, C, N, device):
    """the caller-owned buffers of mtt_det_nms_seg"""
    i32 = dict(dtype=torch.int32, device=device)
    return dict(seg_n=torch.empty(B, C, **i32), seg_idx=torch.empty(B, C, N, **i32), kept_n=torch.empty(B, C, **i32),
                kept=torch.empty(B, C, N, **i32), ws=torch.empty((_lib.det_nms_ws_bytes(B, C, N) + 7) // 8, dtype=torch.int64, device=device))


def buffers(B, C, geo, max_per_img, device):
    """every buffer the four entry points write, uninitialised"""
    N, P = geo['N'], geo['key_off'][-1]
    check_limits(N, C)
    f32, i32 = dict(dtype=torch.float32, device=device), dict(dtype=torch.int32, device=device)
    packed = torch.empty(B * max_per_img * OUT_COLS + B, **f32)              # rows, then count[B] (int32 bit patterns)
    bufs = dict(keys=torch.empty(B, P, **f32), sel=torch.empty(B, N, **i32), box9=torch.empty(B, N, 9, **f32), cen2d=torch.empty(B, N, 3, **f32),
                box2d=torch.empty(B, N, 4, **f32), nmsbox=torch.empty(B, N, 5, **f32), dircls=torch.empty(B, N, 3, **i32),
                scores=torch.empty(B, N, C, **f32), packed=packed, out=packed[:B * max_per_img * OUT_COLS],
                count=packed[B * max_per_img * OUT_COLS:].view(torch.int32))
    bufs.update(nms_buffers(B, C, N, device))
    return bufs


def run(maps, geo, bufs, B, C, inv, img_size, *, dir_offset, score_thr, nms_thr, rotated, max_per_img):
    """maps = (cls, bbox, dir, ctr) per-level contiguous NCHW fp32 lists; inv [B, 16], img_size [B, 2] fp32 on the device"""
    cls, bbox, dirs, ctr = maps
    kw = dict(geo)
    kw.update({k: v for k, v in bufs.items() if k != 'packed'})
    kw.update(cls=list(cls), bbox=list(bbox), dir=list(dirs), ctr=list(ctr), B=B, C=C, inv=inv, img_size=img_size, rotated=1 if rotated else 0,
              max_per_img=int(max_per_img), dir_offset=float(dir_offset), score_thr=float(score_thr), nms_thr=float(nms_thr))
    for name in ("det_select", "det_decode", "det_nms_seg", "det_collect"):
        ops.call(name, **kw)
    return kw
