"""Base property calculators — reference pynbodyext/properties/base.py.

``ParamSum(parameter)``, ``ParamContain(frac, cal_key, parameter)`` (alias
``ParameterContain``), ``VolumeDensity(rmax, parameter, rmin)``,
``SurfaceDensity(rmax, rmin, parameter)`` and
``RadiusAtSurfaceDensity(target, parameter, mode, r_key, eps)`` with the
reference's ``calculate`` on the host.

Device route (MI355X): ``ParamSum("mass")`` is the mass group of the
property pass (csrc/property.hip); the two densities of ``"mass"`` are the
same pass with the scope's predicate ANDed with an Annulus / an rxy band
(two region clauses / one, csrc/region.h); ``ParamContain`` by ``"r"`` / ``"rxy"``
with mass weights is the fused selection followed by the containment of its
whole x (csrc/profile.hip, pbx_profile_contain): the stable sort by radius,
the sequential cumulative mass, np.interp — the reference's values bit for
bit, with ties in index order.  ``RadiusAtSurfaceDensity`` by ``"r"`` /
``"rxy"`` with mass weights is the same selection and sort followed by the
cumulative table kept on the handle (pbx_profile_cum_build) and one launch
that scans the 256 radii and bisects (pbx_profile_cum_solve); the device
squares radii with the product where the host's ``**2`` on scalars is libm
``pow``, so the two routes agree bit for bit whenever no decision of the scan
or the bisection hangs on one ulp of a squared radius.
"""
from __future__ import annotations

from typing import Any

import numpy as np

from .._pyn import SimArray
from ..calculate import CalculatorBase, Param, PropertyBase, and_specs
from ..filters import Annulus, BandPass
from . import _device as dev

__all__ = ["PropertyBase", "ParamSum", "ParamContain", "ParameterContain", "VolumeDensity",
           "SurfaceDensity", "RadiusAtSurfaceDensity"]


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
                                  ndim=3 if params.cal_key == "r" else 2, frame=frame,
                                  region=spec.get("region"))
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


class _DensityPass:
    """The mass group of one property pass divided by a volume or an area."""

    device_groups = dev.MASS

    def __init__(self, extent: float, dim: int):
        self.extent, self.dim = extent, dim

    def finish(self, n_kept, sums, sim):
        return _density(sums[0], self.extent, "mass", self.dim, sim)


def _density(total, extent, parameter, dim, sim) -> SimArray:
    with np.errstate(all="ignore"):  # (an empty shell: x/0 as numpy gives)
        value = np.float64(total) / np.float64(extent)
    return SimArray(value, sim._unit_of(parameter) / sim._unit_of("pos") ** dim, sim=sim.ancestor)


@PropertyBase.dataclass
class VolumeDensity(PropertyBase):
    """Mean volume density of the shell rmin <= r < rmax
    (reference properties/base.py:121-142): the sum of ``parameter`` over
    ``Annulus(rmin, rmax)`` divided by the Annulus volume."""

    rmax: Param[float] = Param(field_name="pos")
    parameter: str = "mass"
    rmin: Param[float] = Param(default=0.0, field_name="pos")

    def calculate(self, sim, params=None):
        selector = Annulus(params.rmin, params.rmax)
        param_sum = np.asarray(sim[selector][params.parameter]).sum()
        return _density(param_sum, selector.volume(sim), params.parameter, 3, sim)

    def device_plan(self, source, spec, params):
        if params.parameter != "mass":
            return None
        selector = Annulus(params.rmin, params.rmax)
        scoped = and_specs(spec, selector.device_spec(source))
        if scoped is None:
            return None
        return dev.moments_plan(_DensityPass(selector.volume(source), 3), source, scoped)


@PropertyBase.dataclass
class SurfaceDensity(PropertyBase):
    """Mean surface density of the ring rmin < rxy < rmax (reference
    properties/base.py:144-169): the sum of ``parameter`` over
    ``BandPass("rxy", rmin, rmax)`` divided by pi (rmax^2 - rmin^2)."""

    rmax: Param[float] = Param(field_name="pos")
    rmin: Param[float] = Param(default=0.0, field_name="pos")
    parameter: str = "mass"

    def calculate(self, sim, params=None):
        selector = BandPass("rxy", params.rmin, params.rmax)
        param_sum = np.asarray(sim[selector][params.parameter]).sum()
        area = np.pi * (params.rmax ** 2 - params.rmin ** 2)
        return _density(param_sum, area, params.parameter, 2, sim)

    def device_plan(self, source, spec, params):
        if params.parameter != "mass":
            return None
        selector = BandPass("rxy", params.rmin, params.rmax)
        scoped = and_specs(spec, selector.device_spec(source))
        if scoped is None:
            return None
        area = np.pi * (params.rmax ** 2 - params.rmin ** 2)
        return dev.moments_plan(_DensityPass(area, 2), source, scoped)


@PropertyBase.dataclass
class RadiusAtSurfaceDensity(PropertyBase):
    """Radius where the surface density reaches a target value (reference
    properties/base.py:172-284).

    In ``mode='shell'`` the surface density is measured in the shell
    ``[r - eps/2, r + eps/2]``; in ``mode='total'`` it is
    ``Sigma(<r) = M(<r) / (pi r^2)``.  The first sign change of
    ``Sigma - target`` along 256 radii between the innermost and the
    outermost particle brackets the root; 80 bisection steps refine it.

    target: a number in the snapshot's units of ``parameter`` per area, a
    unit string, a one-element array or a dynamic value."""

    target: Param[float] = Param()
    parameter: str = "mass"
    mode: str = "shell"
    r_key: str = "rxy"
    eps: float = 0.01

    def resolve_dynamic_params(self, ctx, input):
        # the target is a surface density: _target_value converts it, not the
        # units of a field
        v = self.target
        if isinstance(v, CalculatorBase):
            v = ctx.public_value(v, input)
        elif callable(v):
            v = v(input.active_sim)
        return {"target": v}

    def _target_value(self, sim, params=None):
        unit_of = getattr(sim, "_unit_of", None)  # (the unit table: a frame view derives pos on demand)
        if unit_of is not None:
            surf_units = unit_of(params.parameter) / unit_of("pos") ** 2
        else:
            surf_units = sim[params.parameter].units / sim["pos"].units ** 2
        raw_target = params["target"]
        return self._in_sim_units(raw_target, params.parameter, sim, target_units=surf_units)

    @staticmethod
    def _sigma_at_radius(r_val: float, r_sorted: np.ndarray, m_cum: np.ndarray, eps: float,
                         mode: str) -> float:
        if r_val <= 0:
            return 0.0

        if mode == "total":
            hi = np.searchsorted(r_sorted, r_val, side="right")
            if hi <= 0:
                return 0.0
            m_inside = m_cum[hi - 1]
            area = np.pi * (r_val ** 2)
            return 0.0 if area <= 0 else float(m_inside / area)

        rin = max(r_val - 0.5 * eps, 0.0)
        rout = r_val + 0.5 * eps
        if rout <= 0:
            return 0.0

        lo = np.searchsorted(r_sorted, rin, side="left")
        hi = np.searchsorted(r_sorted, rout, side="right")

        if hi <= 0 or hi <= lo:
            return 0.0

        m_shell = m_cum[hi - 1] - (m_cum[lo - 1] if lo > 0 else 0.0)
        area_shell = np.pi * (rout ** 2 - rin ** 2)
        return 0.0 if area_shell <= 0 else float(m_shell / area_shell)

    def calculate(self, sim, params=None):
        r_arr = sim[params.r_key]
        m_arr = sim[params.parameter]

        pos_units = sim["pos"].units
        mass_units = sim[params.parameter].units

        r_vals = np.asarray(r_arr.in_units(pos_units))
        m_vals = np.asarray(m_arr.in_units(mass_units))

        idx = np.argsort(r_vals)
        r_sorted = r_vals[idx]
        m_sorted = m_vals[idx]
        m_cum = np.cumsum(m_sorted)

        r_min = float(r_sorted[0])
        r_max = float(r_sorted[-1])
        if r_max <= r_min:
            raise ValueError("Degenerate radius distribution")

        target = self._target_value(sim, params)

        sample_grid = np.linspace(max(r_min, params.eps), r_max, 256)
        sigma_grid = np.array(
            [self._sigma_at_radius(r, r_sorted, m_cum, params.eps, params.mode) for r in sample_grid],
            dtype=float)

        diff = sigma_grid - target
        sign_changes = np.where(np.signbit(diff[:-1]) != np.signbit(diff[1:]))[0]
        if len(sign_changes) == 0:
            raise ValueError("Could not bracket target surface density")

        left = float(sample_grid[sign_changes[0]])
        right = float(sample_grid[sign_changes[0] + 1])

        for _ in range(80):
            mid = 0.5 * (left + right)
            sigma_mid = self._sigma_at_radius(mid, r_sorted, m_cum, params.eps, params.mode)
            if abs(sigma_mid - target) < 1e-10:
                left = right = mid
                break
            sigma_left = self._sigma_at_radius(left, r_sorted, m_cum, params.eps, params.mode)
            if (sigma_left - target) * (sigma_mid - target) <= 0:
                right = mid
            else:
                left = mid

        return _contained(0.5 * (left + right), pos_units, sim)

    def device_plan(self, source, spec, params):
        if params.r_key not in ("r", "rxy") or params.parameter != "mass":
            return None
        eps = params.eps
        if not isinstance(eps, (int, float)) or not np.isfinite(eps) or not eps > 0:
            return None
        base, frame = dev.unframe(source)  # (a FrameView: the handle reads its base in its frame)
        arrs = dev.snapshot_arrays(base, ("pos", "mass"))
        if arrs is None:
            return None
        target = self._target_value(source, params)
        if not np.isfinite(target):
            return None
        mode = "total" if params.mode == "total" else "shell"

        def run():
            from ..profiles._device import SRC_W, DeviceBins

            d = DeviceBins.select(arrs["pos"], arrs["mass"], sphere=spec.get("sphere"),
                                  families=spec.get("families"),
                                  ndim=3 if params.r_key == "r" else 2, frame=frame,
                                  region=spec.get("region"))
            try:
                if d.n == 0:  # r_sorted[0] of the reference
                    raise IndexError("index 0 is out of bounds for axis 0 with size 0")
                r_min, r_max, _ = d.cum_build(weights=SRC_W)
                if r_max <= r_min:
                    raise ValueError("Degenerate radius distribution")
                grid = np.linspace(max(r_min, eps), r_max, 256)
                radius, info = d.cum_solve(target, grid, mode=mode, eps=eps)
                if info[0] != 0:
                    raise ValueError("Could not bracket target surface density")
            finally:
                d.close()
            return _contained(radius, source._unit_of("pos"), source)

        return run
