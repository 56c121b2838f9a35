"""TEST INFRASTRUCTURE ONLY — empty placeholders for the cityscapesscripts names the reference's data/cityscapes3d.py imports at module
level.  Only load_det uses them, and the fixture never asks for the 3ddet task."""
