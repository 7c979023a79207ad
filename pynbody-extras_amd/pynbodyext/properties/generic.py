"""Generic property calculators — reference pynbodyext/properties/generic.py.

Centres, bulk velocity, angular momentum, kappa_rot, the virial radius, the
spin parameter and the bar pattern speed, with the reference's numpy
``calculate`` on the host.  VirialRadius and SpinParam call pynbody's
``virial_radius`` / ``spin_parameter`` when pynbody is installed and their
restatements in simcore otherwise.  CenPos("pot" / "hyb") is not provided.

Device route (MI355X): each property names the sum groups it needs
(``device_groups``, include/pbx.h PBX_PROP_*) and applies the reference's
final arithmetic to the count and the 18 sums in ``finish``; the sums come
from one pass over the root snapshot's pos / vel / mass with the Sphere /
family predicate applied in the same pass (csrc/property.hip).
CenPos("ssc") runs the shrinking-sphere loop over data that stays on the
device when the scope has no Sphere or region of its own.  The value's ``.sim`` is the
root snapshot there (the masked sub-snapshot is never built).
VirialRadius computes its target density on the host and hands the bisection
to the library, which decides several levels per pass of the enclosed-mass
kernel (pbx_property_virial_radius); SpinParam takes M and L from the
MASS | ANGMOM pass and R from that kernel's extrema.
"""
from __future__ import annotations

from typing import Any

import numpy as np

from .._pyn import HAVE_PYNBODY, SimArray, shrink_sphere_center, spin_parameter, virial_radius
from ..calculate import PropertyBase
from ..simcore import shrink_sphere_r0, spin_from_sums, virial_target_density
from . import _device as dev

__all__ = ["CenPos", "CenVel", "AngMomVec", "KappaRot", "KappaRotMean", "VirialRadius",
           "SpinParam", "PatternSpeed"]


class _MomentProperty(PropertyBase):
    """A property that is final arithmetic on the sums of the device pass."""

    device_groups = 0

    def finish(self, n_kept: int, sums: np.ndarray, sim):
        raise NotImplementedError

    def device_plan(self, source, spec, params):
        return dev.moments_plan(self, source, spec)


def _ratio(num, den):
    with np.errstate(all="ignore"):  # (nothing kept: 0/0 is NaN, as the host route gives)
        return np.asarray(num, dtype=np.float64) / np.float64(den)


@PropertyBase.dataclass
class CenPos(_MomentProperty):
    """Center position property: "com" (centre of mass) or "ssc"
    (shrinking-sphere centre)."""

    mode: str = "ssc"

    device_groups = dev.MASS | dev.COM

    def __post_init__(self) -> None:
        if self.mode not in ("ssc", "com", "pot", "hyb"):
            raise ValueError(f"Invalid mode: {self.mode}. Expected one of ['ssc', 'com', 'pot', 'hyb'].")
        if self.mode in ("pot", "hyb"):
            raise NotImplementedError(f"CenPos mode {self.mode!r} is not provided "
                                      "(it needs the potential / pynbody's hybrid_center)")

    def calculate(self, sim, params: Any = None):
        if params.mode == "com":
            cen = sim.mean_by_mass("pos")
        elif params.mode == "ssc":
            cen = shrink_sphere_center(sim)
        else:
            raise ValueError(f"Invalid mode: {params.mode}. Expected one of ['ssc', 'com', 'pot', 'hyb'].")
        if isinstance(cen, SimArray):
            cen.sim = sim
        return cen

    def finish(self, n_kept, sums, sim):
        return SimArray(_ratio(sums[1:4], sums[0]), sim._unit_of("pos"), sim=sim)

    def device_plan(self, source, spec, params):
        if params.mode == "com":
            return dev.moments_plan(self, source, spec)
        if params.mode != "ssc" or spec.get("sphere") is not None or spec.get("region"):
            return None
        # (inside a frame the shrinking sphere runs on the host: a FrameView
        # is no root snapshot, pbx_property_shrink_center takes no frame)
        arrs = dev.snapshot_arrays(source, ("pos", "mass"))
        if arrs is None:
            return None
        families = spec.get("families")

        def run():
            # the initial radius, numpy on the host: (x.max() - x.min()) / 2 of
            # the active particles
            x = arrs["pos"][:, 0]
            if families is not None:
                x = np.concatenate([x[a:b] for a, b in families]) if families else x[:0]
            r0 = float((x.max() - x.min()) / 2)
            cen, _, _ = dev.shrink_center(arrs["pos"], arrs["mass"], r0=r0, shrink_factor=0.7,
                                          min_particles=100, families=families)
            return SimArray(cen, source["pos"].units, sim=source)

        return run


@PropertyBase.dataclass
class CenVel(_MomentProperty):
    """Center velocity property"""

    mode: str = "com"

    device_groups = dev.MASS | dev.COV

    def __post_init__(self) -> None:
        if self.mode != "com":
            raise ValueError(f"Invalid mode: {self.mode}. Expected 'com'.")

    def calculate(self, sim, params: Any = None):
        if params.mode == "com":
            cen = sim.mean_by_mass("vel")
        else:
            raise ValueError(f"Invalid mode: {params.mode}. Expected one of ['com'].")
        if isinstance(cen, SimArray):
            cen.sim = sim
        return cen

    def finish(self, n_kept, sums, sim):
        return SimArray(_ratio(sums[4:7], sums[0]), sim._unit_of("vel"), sim=sim)


@PropertyBase.dataclass
class AngMomVec(_MomentProperty):
    """Angular momentum vector property"""

    device_groups = dev.ANGMOM

    def calculate(self, sim, params: Any = None):
        mass = sim["mass"].reshape((len(sim["mass"]), 1))
        pos = sim["pos"]
        vel = sim["vel"]

        cross = np.cross(pos, vel)
        angmom = (mass * cross).sum(axis=0)

        angmom.units = sim["mass"].units * sim["pos"].units * sim["vel"].units
        return angmom

    def finish(self, n_kept, sums, sim):
        units = sim._unit_of("mass") * sim._unit_of("pos") * sim._unit_of("vel")
        return SimArray(sums[7:10].copy(), units, sim=sim)


@PropertyBase.dataclass
class KappaRot(_MomentProperty):
    """Fraction of kinetic energy in ordered rotation, eq. (1) of Sales et
    al. 2010, MNRAS, 409, 1541."""

    device_groups = dev.KAPPA

    def calculate(self, sim, params: Any = None) -> float:
        with np.errstate(all="ignore"):  # (0/0 on the z axis is NaN, kept)
            Krot = np.sum(0.5 * sim["mass"] * (sim["vcxy"] ** 2))
            K = np.sum(sim["mass"] * sim["ke"])
            return float(Krot / K)

    def finish(self, n_kept, sums, sim) -> float:
        return float(_ratio(sums[10], sums[11]))


@PropertyBase.dataclass
class KappaRotMean(_MomentProperty):
    """Mean over the particles of (0.5 * vcxy^2) / ke."""

    device_groups = dev.KAPPA_MEAN

    def calculate(self, sim, params: Any = None) -> float:
        with np.errstate(all="ignore"):
            krot = 0.5 * sim["vcxy"] ** 2
            ke = sim["ke"]
            ratio = krot / ke
            return float(np.mean(ratio)) if len(ratio) else float("nan")

    def finish(self, n_kept, sums, sim) -> float:
        return float(_ratio(sums[12], n_kept))


def _raise_empty():
    """numpy's error for the max of nothing: what the host routes raise when
    the scope keeps no particle (``sim["x"].max()``, ``sim["r"].max()``)."""
    np.empty(0).max()


@PropertyBase.dataclass
class VirialRadius(PropertyBase):
    """Virial radius property: the radius inside which the mean density is
    ``overdensity`` times the critical ("critical") or the mean matter
    ("matter") density at the snapshot's redshift.  The snapshot is taken as
    centred on the origin; it reads ``sim.properties`` (h, omegaM0, omegaL0,
    z)."""

    overdensity: float = 178.
    rho_def: str = "critical"

    NITER_MAX = 200  # pynbody.util.bisect's default

    def __post_init__(self) -> None:
        if self.rho_def not in ("critical", "matter"):
            raise ValueError(f"Invalid rho_def: {self.rho_def}. Expected one of ['critical', 'matter'].")

    def calculate(self, sim, params: Any = None) -> float:
        return virial_radius(sim, overden=params.overdensity, rho_def=params.rho_def)

    def device_plan(self, source, spec, params):
        base, frame = dev.unframe(source)  # (a FrameView: the pass reads its base in its frame)
        arrs = dev.snapshot_arrays(base, ("pos", "mass"))
        if arrs is None:
            return None
        target_rho = virial_target_density(source, params.overdensity, params.rho_def)
        if not (np.isfinite(target_rho) and target_rho > 0):
            return None

        def run():
            radius, _, _, n_kept, converged = dev.virial_radius(
                arrs["pos"], arrs["mass"], target_rho=target_rho, eta=1.0e-3 * target_rho,
                niter_max=self.NITER_MAX, sphere=spec.get("sphere"),
                families=spec.get("families"), frame=frame, region=spec.get("region"))
            if n_kept == 0:
                _raise_empty()
            if not converged:
                raise ValueError("Bisection algorithm did not converge")
            return radius

        return run


@PropertyBase.dataclass
class SpinParam(PropertyBase):
    """The spin parameter lambda' of eq. (5) of Bullock et al. 2001, MNRAS,
    321, 559: J / (sqrt(2) M V R) with V = sqrt(G M / R).  The halo is taken
    as centred on the origin with zero bulk velocity."""

    def calculate(self, sim, params: Any = None) -> float:
        return spin_parameter(sim)

    def device_plan(self, source, spec, params):
        base, frame = dev.unframe(source)
        arrs = dev.snapshot_arrays(base, ("pos", "vel", "mass"))
        if arrs is None:
            return None
        scope = dict(sphere=spec.get("sphere"), families=spec.get("families"), frame=frame,
                     region=spec.get("region"))

        def run():
            # M and L from the MASS | ANGMOM pass, R from the extrema of the
            # enclosed pass (no thresholds)
            n_kept, sums = dev.moments(arrs["pos"], arrs["vel"], arrs["mass"],
                                       groups=dev.MASS | dev.ANGMOM, **scope)
            if n_kept == 0:
                _raise_empty()
            _, _, _, ext = dev.enclosed(arrs["pos"], arrs["mass"], **scope)
            return spin_from_sums(sums[0], sums[7:10], ext[6], source)

        return run


@PropertyBase.dataclass
class PatternSpeed(_MomentProperty):
    """Pattern speed about z of a disk in the x-y plane, eq. 46 of Pfenniger
    & Romero-Gómez 2023, A&A, 673, A36."""

    device_groups = dev.PATTERN

    def calculate(self, sim, params: Any = None):
        with np.errstate(all="ignore"):
            Ixx = (sim["mass"]*sim["x"]*sim["x"]).sum()
            Iyy = (sim["mass"]*sim["y"]*sim["y"]).sum()
            Ixy = (sim["mass"]*sim["x"]*sim["y"]).sum()
            I_minus = 1/2*(Ixx-Iyy)
            d_Ixy = (sim["mass"]*(sim["x"]*sim["vy"]+sim["y"]*sim["vx"])).sum()
            d_I_minus = (sim["mass"]*(sim["x"]*sim["vx"]-sim["y"]*sim["vy"])).sum()

            omega_Iz = 1/2*(I_minus*d_Ixy-d_I_minus*Ixy)/(I_minus*I_minus+Ixy*Ixy)
        if not HAVE_PYNBODY:  # (the stand-in's arrays do not derive units through arithmetic)
            omega_Iz.units = sim["vel"].units / sim["pos"].units
        omega_Iz.sim = sim.ancestor
        return omega_Iz

    def finish(self, n_kept, sums, sim):
        Ixx, Iyy, Ixy, d_Ixy, d_I_minus = (np.float64(v) for v in sums[13:18])
        with np.errstate(all="ignore"):
            I_minus = 1/2*(Ixx-Iyy)
            omega_Iz = 1/2*(I_minus*d_Ixy-d_I_minus*Ixy)/(I_minus*I_minus+Ixy*Ixy)
        return SimArray(omega_Iz, sim._unit_of("vel") / sim._unit_of("pos"), sim=sim.ancestor)
