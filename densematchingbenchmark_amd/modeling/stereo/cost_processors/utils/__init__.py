from .hw_hourglass import HWHourglass  # noqa: F401
