"""TEST INFRASTRUCTURE ONLY — imageio.imread for the reference's data/cityscapes3d.py: the decoded PNG as a writable numpy array."""
import numpy as np
from PIL import Image


def imread(path):
    return np.array(Image.open(path))
