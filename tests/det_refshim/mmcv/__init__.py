"""mmcv stand-in (restated layers only; see tests/det_refshim/__init__.py)."""
