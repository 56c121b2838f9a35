"""mmcv.runner.BaseModule / auto_fp16 as the head uses them: an nn.Module that keeps init_cfg, and a no-op decorator (fp32 only)."""
import torch.nn as nn


class BaseModule(nn.Module):
    def __init__(self, init_cfg=None):
        super().__init__()
        self.init_cfg = init_cfg


def auto_fp16(apply_to=None, out_fp32=False):
    def deco(fn):
        return fn
    return deco
