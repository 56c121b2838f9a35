"""TEST INFRASTRUCTURE ONLY — the three torchvision transforms the reference's data/cityscapes3d.py composes, restated from their
documentation for the one input it gives them (a uint8 [H, W, C] numpy array):

  ToTensor    [C, H, W] float32, the bytes divided by 255
  Normalize   (t - mean[c]) / std[c] with mean and std as float32 tensors
  Compose     the transforms in order
"""
import numpy as np
import torch


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class ToTensor:
    def __call__(self, pic):
        if not (isinstance(pic, np.ndarray) and pic.dtype == np.uint8 and pic.ndim == 3):
            raise TypeError("the stand-in takes uint8 [H, W, C] arrays only")
        return torch.from_numpy(np.ascontiguousarray(pic.transpose(2, 0, 1))).to(torch.float32).div(255)


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        mean = torch.as_tensor(self.mean, dtype=t.dtype).view(-1, 1, 1)
        std = torch.as_tensor(self.std, dtype=t.dtype).view(-1, 1, 1)
        return t.clone().sub_(mean).div_(std)
