"""Property calculators (reference pynbodyext/properties)."""

from .base import (
    ParamContain,
    ParameterContain,
    ParamSum,
    PropertyBase,
    RadiusAtSurfaceDensity,
    SurfaceDensity,
    VolumeDensity,
)
from .generic import (
    AngMomVec,
    CenPos,
    CenVel,
    KappaRot,
    KappaRotMean,
    PatternSpeed,
    SpinParam,
    VirialRadius,
)

__all__ = [
    "PropertyBase",
    "ParamSum",
    "ParamContain",
    "ParameterContain",
    "VolumeDensity",
    "SurfaceDensity",
    "RadiusAtSurfaceDensity",
    "KappaRot",
    "KappaRotMean",
    "CenPos",
    "CenVel",
    "AngMomVec",
    "PatternSpeed",
    "VirialRadius",
    "SpinParam",
]
