"""Property calculators (reference pynbodyext/properties)."""

from .base import ParamContain, ParameterContain, ParamSum, PropertyBase
from .generic import AngMomVec, CenPos, CenVel, KappaRot, KappaRotMean, PatternSpeed

__all__ = [
    "PropertyBase",
    "ParamSum",
    "ParamContain",
    "ParameterContain",
    "KappaRot",
    "KappaRotMean",
    "CenPos",
    "CenVel",
    "AngMomVec",
    "PatternSpeed",
]
