CRS_V, CRS_C, CRS_S = 0, 1, 2


class Camera:
    """placeholder: never instantiated by the fixture"""


class Box3dImageTransform:
    """placeholder: never instantiated by the fixture"""
