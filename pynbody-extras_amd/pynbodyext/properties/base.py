"""Base property calculators — reference pynbodyext/properties/base.py.

``ParamSum(parameter)`` and ``ParamContain(frac, cal_key, parameter)`` (alias
``ParameterContain``) with the reference's ``calculate`` on the host.  The
density-style properties of the reference module (VolumeDensity,
SurfaceDensity, RadiusAtSurfaceDensity) need Annulus / BandPass filters and
are not provided.

Device route (MI355X): ``ParamSum("mass")`` is the mass group of the
property pass (csrc/property.hip); ``ParamContain`` by ``"r"`` / ``"rxy"``
with mass weights is the fused selection followed by the containment of its
whole x (csrc/profile.hip, pbx_profile_contain): the stable sort by radius,
the sequential cumulative mass, np.interp — the reference's values bit for
bit, with ties in index order.
"""
from __future__ import annotations

from typing import Any

import numpy as np

from .._pyn import SimArray
from ..calculate import Param, PropertyBase
from . import _device as dev

__all__ = ["PropertyBase", "ParamSum", "ParamContain", "ParameterContain"]


def _normalize_frac(frac: Any) -> tuple[np.ndarray, bool]:
    frac_array = np.asarray([frac] if isinstance(frac, (int, float, np.floating)) else frac, dtype=float)
    if frac_array.ndim != 1:
        raise ValueError("frac must be a scalar or 1D sequence.")
    if not np.all((frac_array > 0) & (frac_array < 1)):
        raise ValueError(f"frac values must be between 0 and 1, got {frac_array}.")
    return frac_array, frac_array.size == 1 and isinstance(frac, (int, float, np.floating))


def _contained(result, key_units, sim) -> SimArray:
    contained = SimArray(result)
    if key_units is not None:
        contained.units = key_units
    if hasattr(sim, "ancestor"):
        contained.sim = sim.ancestor
    return contained


@PropertyBase.dataclass
class ParamContain(PropertyBase):
    """Containment radius for one or more cumulative fractions
    (reference properties/base.py:60-103).

    frac: cumulative fraction(s) in (0, 1), or a dynamic value; cal_key: the
    field to sort by; parameter: the weight field of the cumulative sum.
    The historical positional order ``ParamContain("r", 0.5)`` (field first)
    is accepted as well, and so is the field alone, ``ParamContain("r")``.
    """

    frac: Param[float] = Param(default=0.5)
    cal_key: str = "r"
    parameter: str = "mass"

    def __post_init__(self) -> None:
        if isinstance(self.frac, str) and not isinstance(self.cal_key, str):
            self.frac, self.cal_key = self.cal_key, self.frac
        elif isinstance(self.frac, str):  # ParamContain("r"): the field alone, half of it
            self.frac, self.cal_key = 0.5, self.frac

    def calculate(self, sim, params=None):
        frac = params.frac
        frac_array, frac_is_scalar = _normalize_frac(frac)
        key = sim[params.cal_key]
        weight = sim[params.parameter]
        order = np.argsort(np.asarray(key))
        key_sorted = np.asarray(key)[order]
        weight_sorted = np.asarray(weight)[order]
        cumulative = np.cumsum(weight_sorted)
        denom = float(cumulative[-1] - cumulative[0])
        if denom <= 0.0:
            raise ValueError(f"Non-positive total {params.parameter!r}; cannot compute containment radius.")
        cumulative = (cumulative - cumulative[0]) / denom
        values = np.interp(frac_array, cumulative, key_sorted)
        result: float | np.ndarray = float(values[0]) if frac_is_scalar else values
        return _contained(result, getattr(key, "units", None), sim)

    def device_plan(self, source, spec, params):
        if params.cal_key not in ("r", "rxy") or params.parameter != "mass":
            return None
        base, frame = dev.unframe(source)  # (a FrameView: the handle reads its base in its frame)
        arrs = dev.snapshot_arrays(base, ("pos", "mass"))
        if arrs is None:
            return None
        frac_array, frac_is_scalar = _normalize_frac(params.frac)

        def run():
            from ..profiles._device import SRC_W, DeviceBins

            d = DeviceBins.select(arrs["pos"], arrs["mass"], sphere=spec.get("sphere"),
                                  families=spec.get("families"),
                                  ndim=3 if params.cal_key == "r" else 2, frame=frame)
            try:
                if d.n == 0:  # cumulative[-1] of the reference
                    raise IndexError("index -1 is out of bounds for axis 0 with size 0")
                values, denom = d.contain(frac_array, weights=SRC_W)
                if d.n < 2 or denom <= 0.0:
                    raise ValueError(f"Non-positive total {params.parameter!r}; "
                                     "cannot compute containment radius.")
            finally:
                d.close()
            result = float(values[0]) if frac_is_scalar else values
            return _contained(result, source._unit_of(params.cal_key), source)

        return run


ParameterContain = ParamContain


@PropertyBase.dataclass
class ParamSum(PropertyBase):
    """Sum a simulation field (reference properties/base.py:106-119)."""

    parameter: str

    device_groups = dev.MASS

    def calculate(self, sim: Any, params: Any = None) -> Any:
        return sim[params.parameter].sum()

    def finish(self, n_kept, sums, sim):
        return SimArray(sums[0], sim._unit_of("mass"), sim=sim)

    def device_plan(self, source, spec, params):
        if params.parameter != "mass":
            return None
        return dev.moments_plan(self, source, spec)
