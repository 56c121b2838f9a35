"""TEST INFRASTRUCTURE ONLY — imageio.imwrite for the reference's evaluation/evaluate_utils.py: records (path, a copy of the array) in the
same list as the cv2 stand-in instead of encoding a file."""
import cv2


def imwrite(path, arr):
    return cv2.imwrite(path, arr)
