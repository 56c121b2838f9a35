"""TEST INFRASTRUCTURE ONLY — see transforms/__init__.py."""
from . import transforms  # noqa: F401
