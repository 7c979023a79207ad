"""Particle selection filters.

The nine filters of the reference (pynbodyext/filters/filt.py: ``Sphere``,
``FamilyFilter``, ``Cuboid``, ``Disc``, ``Annulus``, ``SolarNeighborhood``,
``BandPass``, ``HighPass``, ``LowPass``) with its constructor signatures and
defaults and the mask semantics of pynbody.filt: every comparison strict, no
periodic wrap, ``Annulus`` = ``Sphere(r2) & ~Sphere(r1)`` (the inner boundary
is kept), ``SolarNeighborhood`` = ``Disc(r2, h) & ~Disc(r1, h)``.

Besides the host mask (``build_mask``, plain numpy) each filter describes
itself to the device (``device_spec``): a Sphere takes the selection's sphere
slot, a family its index range, everything else becomes clauses of the
pass's region (pynbodyext/region.py, csrc/region.h), so a profile or a
property behind ``Disc & FamilyFilter`` is selected and measured in one GPU
pass.  ``&`` concatenates clauses (a second Sphere becomes one), ``~``
negates a single clause; more than 8 clauses, ``|`` of anything but
families, and a ``BandPass`` on a field other than x, y, z, r, rxy take the
host route.
"""
from __future__ import annotations

import numpy as np

from .. import region as rg
from .._pyn import filt, get_family
from ..calculate import AndFilter, FilterBase, NotFilter, OrFilter, resolve_value_in_units

__all__ = ["FilterBase", "Sphere", "FamilyFilter", "Cuboid", "Disc", "Annulus", "BandPass",
           "HighPass", "LowPass", "SolarNeighborhood", "AndFilter", "OrFilter", "NotFilter"]


def _value(v, sim, field):
    """A number, a unit string, a callable of the snapshot or a calculator as
    a float in the units of ``sim[field]`` (None stays None)."""
    if callable(v):
        v = v(sim)
    v = resolve_value_in_units(v, sim, field)
    return None if v is None else float(v)


def _centre(cen, sim):
    if callable(cen):
        cen = cen(sim)
    return np.asarray(cen, dtype=np.float64).reshape(3)


class _RegionFilter(FilterBase):
    """A filter that is a conjunction of region clauses of the positions:
    ``clauses(sim)`` is both the host mask and the device description."""

    def clauses(self, sim) -> list:
        raise NotImplementedError

    def build_mask(self, sim, params=None):
        return rg.region_mask(np.asarray(sim["pos"]), self.clauses(sim))

    def device_spec(self, sim):
        return {"region": self.clauses(sim)}


class Sphere(FilterBase):
    """Particles with ((x-cx)^2 + (y-cy)^2) + (z-cz)^2 < radius^2."""

    dynamic_param_specs = {"radius": "pos", "cen": "pos"}

    def __init__(self, radius, cen=(0, 0, 0)):
        self.radius = radius
        self.cen = cen

    def _resolved(self, sim):
        r = self.radius(sim) if callable(self.radius) else self.radius
        c = self.cen(sim) if callable(self.cen) else self.cen
        r = resolve_value_in_units(r, sim, "pos")
        c = np.asarray(c, dtype=np.float64).reshape(3)
        return c, float(r)

    def build_mask(self, sim, params=None):
        cen, radius = self._resolved(sim)
        p = np.asarray(sim["pos"])
        dx = p[:, 0] - cen[0]
        dy = p[:, 1] - cen[1]
        dz = p[:, 2] - cen[2]
        return ((dx * dx + dy * dy) + dz * dz) < radius * radius

    def device_spec(self, sim):
        cen, radius = self._resolved(sim)
        return {"sphere": (cen, radius)}

    def volume(self, sim=None):
        _, radius = self._resolved(sim) if sim is not None else (None, float(self.radius))
        return 4.0 / 3.0 * np.pi * radius ** 3

    def __repr__(self):
        return f"Sphere(radius={self.radius!r}, cen={self.cen!r})"


def _family_slice(sim, fam):
    """The family's contiguous index range in ``sim`` through pynbody's own
    snapshot interface (``SimSnap._get_family_slice``, as the reference's
    chunk.py:186,232 uses it), or None when the members do not form one
    range (e.g. an index-list sub-snapshot) or ``sim`` has no families."""
    get = getattr(sim, "_get_family_slice", None)
    if get is None:
        return None
    sl = get(fam)
    if not isinstance(sl, slice) or sl.step not in (None, 1):
        return None
    start, stop, _ = sl.indices(len(sim))
    return slice(start, max(start, stop))


class FamilyFilter(FilterBase):
    """Particles of one family (dm, gas, star, ...).  The mask is pynbody's
    own ``filt.FamilyFilter(family)(sim)`` (reference filt.py:84-86 delegates
    to it); the device selection takes the family's index range."""

    def __init__(self, family):
        if isinstance(family, str):
            family = get_family(family, False)
        self.family = family

    def _family(self, sim):
        fam = self.family
        if callable(fam) and not hasattr(fam, "name"):
            fam = fam(sim)
        return get_family(fam, False) if isinstance(fam, str) else fam

    def build_mask(self, sim, params=None):
        return np.asarray(filt.FamilyFilter(self._family(sim))(sim), dtype=bool)

    def device_spec(self, sim):
        if callable(self.family) and not hasattr(self.family, "name"):
            return None
        sl = _family_slice(sim, self._family(sim))
        if sl is None:
            return None
        return {"families": [(sl.start, sl.stop)] if sl.stop > sl.start else []}

    def __repr__(self):
        return f"FamilyFilter({getattr(self.family, 'name', self.family)!r})"


class Cuboid(_RegionFilter):
    """Particles with x1 < x < x2, y1 < y < y2, z1 < z < z2.  ``Cuboid(x1)``
    fills y1 = z1 = x1 and x2 = -x1, y2 = -y1, z2 = -z1 (pynbody.filt.Cuboid)."""

    dynamic_param_specs = {k: "pos" for k in ("x1", "y1", "z1", "x2", "y2", "z2")}

    def __init__(self, x1, y1=None, z1=None, x2=None, y2=None, z2=None):
        self.x1, self.y1, self.z1, self.x2, self.y2, self.z2 = x1, y1, z1, x2, y2, z2

    def _resolved(self, sim):
        """The six corners, the missing ones filled as pynbody.filt.Cuboid does."""
        x1, y1, z1, x2, y2, z2 = (_value(getattr(self, k), sim, "pos")
                                  for k in ("x1", "y1", "z1", "x2", "y2", "z2"))
        if y1 is None:
            y1 = x1
        if z1 is None:
            z1 = x1
        if x2 is None:
            x2 = -x1
        if y2 is None:
            y2 = -y1
        if z2 is None:
            z2 = -z1
        return x1, y1, z1, x2, y2, z2

    def clauses(self, sim):
        return [rg.cuboid_clause(*self._resolved(sim))]

    def volume(self, sim=None):
        # (the reference's (x2 - x1) (y2 - y1) (z2 - z1); for a corner left out
        # it multiplies by None, so the filled corners of the mask are used)
        x1, y1, z1, x2, y2, z2 = self._resolved(sim)
        return (x2 - x1) * (y2 - y1) * (z2 - z1)

    def __repr__(self):
        return (f"Cuboid({self.x1!r}, {self.y1!r}, {self.z1!r}, {self.x2!r}, {self.y2!r}, "
                f"{self.z2!r})")


class Disc(_RegionFilter):
    """Particles with (dx*dx + dy*dy) < radius^2 and |dz| < height."""

    dynamic_param_specs = {"radius": "pos", "height": "pos", "cen": "pos"}

    def __init__(self, radius, height, cen=(0, 0, 0)):
        self.radius, self.height, self.cen = radius, height, cen

    def clauses(self, sim):
        return [rg.disc_clause(_centre(self.cen, sim), _value(self.radius, sim, "pos"),
                               _value(self.height, sim, "pos"))]

    def volume(self, sim=None):
        radius, height = _value(self.radius, sim, "pos"), _value(self.height, sim, "pos")
        return 2 * np.pi * radius ** 2 * height

    def __repr__(self):
        return f"Disc(radius={self.radius!r}, height={self.height!r}, cen={self.cen!r})"


class Annulus(_RegionFilter):
    """``Sphere(r2, cen) & ~Sphere(r1, cen)``: r1 is the inner radius, and a
    particle exactly on it is kept."""

    dynamic_param_specs = {"r1": "pos", "r2": "pos", "cen": "pos"}

    def __init__(self, r1, r2, cen=(0, 0, 0)):
        self.r1, self.r2, self.cen = r1, r2, cen

    def clauses(self, sim):
        cen = _centre(self.cen, sim)
        return [rg.sphere_clause(cen, _value(self.r2, sim, "pos")),
                rg.sphere_clause(cen, _value(self.r1, sim, "pos"), negate=True)]

    def volume(self, sim=None):
        r1, r2 = _value(self.r1, sim, "pos"), _value(self.r2, sim, "pos")
        return 4.0 / 3.0 * np.pi * (r2 ** 3 - r1 ** 3)

    def __repr__(self):
        return f"Annulus(r1={self.r1!r}, r2={self.r2!r}, cen={self.cen!r})"


class SolarNeighborhood(_RegionFilter):
    """``Disc(r2, height, cen) & ~Disc(r1, height, cen)``."""

    dynamic_param_specs = {"r1": "pos", "r2": "pos", "height": "pos", "cen": "pos"}

    def __init__(self, r1="5 kpc", r2="10 kpc", height="2 kpc", cen=(0, 0, 0)):
        self.r1, self.r2, self.height, self.cen = r1, r2, height, cen

    def clauses(self, sim):
        cen, h = _centre(self.cen, sim), _value(self.height, sim, "pos")
        return [rg.disc_clause(cen, _value(self.r2, sim, "pos"), h),
                rg.disc_clause(cen, _value(self.r1, sim, "pos"), h, negate=True)]

    def volume(self, sim=None):
        r1, r2 = _value(self.r1, sim, "pos"), _value(self.r2, sim, "pos")
        height = _value(self.height, sim, "pos")
        return 2 * np.pi * height * (r2 ** 2 - r1 ** 2)

    def __repr__(self):
        return (f"SolarNeighborhood(r1={self.r1!r}, r2={self.r2!r}, height={self.height!r}, "
                f"cen={self.cen!r})")


class BandPass(FilterBase):
    """Particles with min < sim[prop] < max.  On x, y, z, r, rxy it is a
    region clause of the positions; on any other field a host mask."""

    def __init__(self, prop, min, max):
        self.prop, self.min, self.max = prop, min, max

    @property
    def dynamic_param_specs(self):
        return {"min": self.prop, "max": self.prop}

    def _bounds(self, sim):
        return _value(self.min, sim, self.prop), _value(self.max, sim, self.prop)

    def build_mask(self, sim, params=None):
        lo, hi = self._bounds(sim)
        if self.prop in rg.BAND_FIELDS and "pos" in sim.keys():
            return rg.clause_mask(np.asarray(sim["pos"]), rg.band_clause(self.prop, lo, hi))
        f = np.asarray(sim[self.prop])
        m = np.ones(len(f), dtype=bool)
        if lo is not None:
            m &= f > lo
        if hi is not None:
            m &= f < hi
        return m

    def device_spec(self, sim):
        if self.prop not in rg.BAND_FIELDS:
            return None
        lo, hi = self._bounds(sim)
        return {"region": [rg.band_clause(self.prop, lo, hi)]}

    def __repr__(self):
        return f"BandPass({self.prop!r}, {self.min!r}, {self.max!r})"


class HighPass(BandPass):
    """Particles with sim[prop] > min."""

    def __init__(self, prop, min):
        super().__init__(prop, min, None)

    def __repr__(self):
        return f"HighPass({self.prop!r}, {self.min!r})"


class LowPass(BandPass):
    """Particles with sim[prop] < max."""

    def __init__(self, prop, max):
        super().__init__(prop, None, max)

    def __repr__(self):
        return f"LowPass({self.prop!r}, {self.max!r})"
