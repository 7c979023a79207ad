"""Property calculators (reference pynbodyext/properties)."""

from .base import (
    ParamContain,
    ParameterContain,
    ParamSum,
    PropertyBase,
    SurfaceDensity,
    VolumeDensity,
)
from .generic import AngMomVec, CenPos, CenVel, KappaRot, KappaRotMean, PatternSpeed

__all__ = [
    "PropertyBase",
    "ParamSum",
    "ParamContain",
    "ParameterContain",
    "VolumeDensity",
    "SurfaceDensity",
    "KappaRot",
    "KappaRotMean",
    "CenPos",
    "CenVel",
    "AngMomVec",
    "PatternSpeed",
]
