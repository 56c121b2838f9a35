class CsBbox3d:
    """placeholder: never instantiated by the fixture"""
