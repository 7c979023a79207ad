"""Shared by tests/test_transforms_cpu.py and tests/test_gpu_transforms.py: a
synthetic disc galaxy, the README's larger example on it, and that example
written out by hand in numpy (any float dtype).  Test infrastructure only.
"""
from __future__ import annotations

import numpy as np

from pynbodyext.filters import FamilyFilter, Sphere
from pynbodyext.properties import AngMomVec, KappaRot, ParamContain
from pynbodyext.simcore import SimSnap, as_unit, calc_faceon_matrix
from pynbodyext.transforms import AlignVec, ShiftPosTo, ShiftVelTo

UNITS = {"pos": "kpc", "vel": "km s**-1", "mass": "Msol"}
N_DM, N_STAR = 8000, 12000
STAR = slice(N_DM, N_DM + N_STAR)

# the known rotation (z-y-x Euler angles), displacement and boost of the disc
ANGLES = (0.7, -1.1, 2.3)
SHIFT = np.array([40.0, -25.0, 10.0])
BOOST = np.array([120.0, -80.0, 30.0])


def euler_matrix(a, b, c) -> np.ndarray:
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    rz = np.array([[ca, -sa, 0.0], [sa, ca, 0.0], [0.0, 0.0, 1.0]])
    ry = np.array([[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cc, -sc], [0.0, sc, cc]])
    return rz @ ry @ rx


def disc_arrays(seed=2024):
    """(pos, vel, mass) of a dark halo (first N_DM) and a cold stellar disc in
    the x-y plane rotating about +z, centred and at rest."""
    rng = np.random.default_rng(seed)
    hr = 20.0 * rng.uniform(0.0, 1.0, N_DM) ** (1.0 / 3.0) / np.sqrt(1.0 - rng.uniform(0, 0.9, N_DM))
    hd = rng.normal(size=(N_DM, 3))
    hpos = hd / np.linalg.norm(hd, axis=1)[:, None] * hr[:, None]
    hvel = rng.normal(scale=100.0, size=(N_DM, 3))
    rad = rng.exponential(3.0, N_STAR)
    phi = rng.uniform(0.0, 2.0 * np.pi, N_STAR)
    spos = np.stack([rad * np.cos(phi), rad * np.sin(phi), rng.normal(scale=0.3, size=N_STAR)], axis=1)
    vc = 200.0 * rad / np.sqrt(rad * rad + 1.0)
    svel = np.stack([-vc * np.sin(phi), vc * np.cos(phi), np.zeros(N_STAR)], axis=1)
    svel += rng.normal(scale=20.0, size=(N_STAR, 3))
    pos = np.concatenate([hpos, spos])
    vel = np.concatenate([hvel, svel])
    mass = np.concatenate([rng.uniform(4.0, 6.0, N_DM), rng.uniform(0.5, 1.5, N_STAR)])
    return pos, vel, mass


def snapshot(pos, vel, mass) -> SimSnap:
    return SimSnap({"pos": np.ascontiguousarray(pos), "vel": np.ascontiguousarray(vel),
                    "mass": np.ascontiguousarray(mass)},
                   families={"dm": slice(0, N_DM), "star": STAR}, units_map=UNITS)


def moved(pos, vel):
    """The disc rotated by the known matrix, displaced and boosted."""
    q = euler_matrix(*ANGLES)
    return pos @ q.T + SHIFT, vel @ q.T + BOOST


def example_transform():
    re = ParamContain("r").filter(Sphere("30 kpc") & FamilyFilter("star"))
    return (ShiftPosTo("ssc")
            .then(ShiftVelTo("com").filter(Sphere(0.5 * re) & FamilyFilter("star")))
            .then(AlignVec(AngMomVec().filter(Sphere(2 * re) & FamilyFilter("star")))))


def example_scope():
    return Sphere("30 kpc") & FamilyFilter("star")


def example():
    """The README's larger example."""
    return KappaRot().filter(example_scope()).transform(example_transform())


# ---------------------------------------------------------------- by hand
def _shift(a, c):
    out = np.empty_like(a)
    out[:, 0], out[:, 1], out[:, 2] = a[:, 0] - c[0], a[:, 1] - c[1], a[:, 2] - c[2]
    return out


def _rotate(a, r):
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    out = np.empty_like(a)
    out[:, 0] = (r[0, 0] * x + r[0, 1] * y) + r[0, 2] * z
    out[:, 1] = (r[1, 0] * x + r[1, 1] * y) + r[1, 2] * z
    out[:, 2] = (r[2, 0] * x + r[2, 1] * y) + r[2, 2] * z
    return out


def _in_sphere(p, radius):
    return ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]) < radius * radius


def _shrink_centre(pos, mass):
    com = (pos.T * mass).sum(axis=1) / mass.sum()
    r = (pos[:, 0].max() - pos[:, 0].min()) / 2
    while True:
        dx, dy, dz = pos[:, 0] - com[0], pos[:, 1] - com[1], pos[:, 2] - com[2]
        keep = ((dx * dx + dy * dy) + dz * dz) < r * r
        if np.count_nonzero(keep) <= 100:
            return com
        com = (pos[keep].T * mass[keep]).sum(axis=1) / mass[keep].sum()
        r *= 0.7


def _half_mass_radius(p, m):
    r = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    order = np.argsort(r)
    rs, cum = r[order], np.cumsum(m[order])
    cum = (cum - cum[0]) / (cum[-1] - cum[0])
    if r.dtype == np.float64:
        return np.interp(np.asarray([0.5]), cum, rs)[0]
    j = np.searchsorted(cum, 0.5, side="right") - 1  # (np.interp is float64 only)
    return rs[j] + (rs[j + 1] - rs[j]) * ((0.5 - cum[j]) / (cum[j + 1] - cum[j]))


def example_by_hand(pos, vel, mass, dtype=np.float64):
    """(kappa_rot, frame parts, final pos, final vel): the example as the
    numpy sequence a user would write, every array rewritten in turn.  In
    float64 each expression is the host route's own, so the values agree bit
    for bit; in longdouble it is the yardstick of the routes' rounding."""
    pos, vel, mass = (np.asarray(a).astype(dtype) for a in (pos, vel, mass))
    star = np.zeros(len(pos), dtype=bool)
    star[STAR] = True
    thirty = dtype(float(as_unit("30 kpc").ratio(as_unit("kpc"))))  # Sphere("30 kpc")'s number
    c = _shrink_centre(pos, mass)
    p1 = _shift(pos, c)
    k = star & _in_sphere(p1, thirty)
    re = _half_mass_radius(p1[k], mass[k])
    k = star & _in_sphere(p1, dtype(float(0.5 * re)) if dtype == np.float64 else 0.5 * re)
    vc = (vel[k].T * mass[k]).sum(axis=-1) / mass[k].sum()
    v1 = _shift(vel, vc)
    k = star & _in_sphere(p1, dtype(float(2 * re)) if dtype == np.float64 else 2 * re)
    ang = (mass[k].reshape((k.sum(), 1)) * np.cross(p1[k], v1[k])).sum(axis=0)
    if dtype == np.float64:
        rot = calc_faceon_matrix(ang, up=AlignVec._safe_up(ang))
    else:
        up = AlignVec._safe_up(ang.astype(np.float64)).astype(dtype)
        vec = ang / np.sqrt((ang * ang).sum())
        q1 = np.cross(up, vec)
        q1 = q1 / np.sqrt((q1 * q1).sum())
        rot = np.stack((q1, np.cross(vec, q1), vec))
    p2, v2 = _rotate(p1, rot), _rotate(v1, rot)
    k = star & _in_sphere(p2, thirty)
    x, y, vx, vy, vz = p2[k, 0], p2[k, 1], v2[k, 0], v2[k, 1], v2[k, 2]
    vcxy = (x * vy - y * vx) / np.sqrt(x * x + y * y)
    ke = 0.5 * ((vx * vx + vy * vy) + vz * vz)
    kappa = np.sum(0.5 * mass[k] * (vcxy ** 2)) / np.sum(mass[k] * ke)
    return kappa, (c, vc, rot), p2, v2
