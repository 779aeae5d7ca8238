from .focal import FocalLoss  # noqa: F401
from .losses import InfoNCELoss  # noqa: F401

__all__ = ["FocalLoss", "InfoNCELoss"]
