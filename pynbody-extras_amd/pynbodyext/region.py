"""The region of a device pass: a conjunction of clauses (include/pbx.h,
pbx_profile_set_region; csrc/region.h).

A clause is ``(kind, negate, params)``: one primitive (sphere, disc, cuboid,
band of x / y / z / r / rxy), optionally negated, with its six constants.
``clause_mask`` is the plain-numpy restatement of the device arithmetic, in
the same operation order (float64, strict comparisons, a negated clause is
``~mask``): the host route of the filters and the oracle of the tests.
"""
from __future__ import annotations

import ctypes

import numpy as np

REGION_MAX = 8
SPHERE, DISC, CUBOID, BAND = 1, 2, 3, 4  # pbx.h PBX_REGION_*
BAND_FIELDS = ("x", "y", "z", "r", "rxy")  # by field code, pbx.h PBX_BAND_*


def sphere_clause(cen, radius, negate=False):
    cx, cy, cz = (float(v) for v in np.asarray(cen, dtype=np.float64).reshape(3))
    radius = float(radius)
    return (SPHERE, bool(negate), (cx, cy, cz, radius * radius, 0.0, 0.0))


def disc_clause(cen, radius, height, negate=False):
    cx, cy, cz = (float(v) for v in np.asarray(cen, dtype=np.float64).reshape(3))
    radius = float(radius)
    return (DISC, bool(negate), (cx, cy, cz, radius * radius, float(height), 0.0))


def cuboid_clause(x1, y1, z1, x2, y2, z2, negate=False):
    return (CUBOID, bool(negate), tuple(float(v) for v in (x1, y1, z1, x2, y2, z2)))


def band_clause(field, lo=None, hi=None, negate=False):
    """``field`` in BAND_FIELDS; lo / hi None: that side is open."""
    code = BAND_FIELDS.index(field)
    return (BAND, bool(negate), (float(code), 0.0 if lo is None else float(lo),
                                 0.0 if hi is None else float(hi),
                                 0.0 if lo is None else 1.0, 0.0 if hi is None else 1.0, 0.0))


def negated(clause):
    kind, neg, params = clause
    return (kind, not neg, params)


def clause_mask(pos, clause) -> np.ndarray:
    """Mask of one clause over (N,3) float64 positions."""
    kind, neg, q = clause
    p = np.asarray(pos, dtype=np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == SPHERE:
            dx, dy, dz = x - q[0], y - q[1], z - q[2]
            m = ((dx * dx + dy * dy) + dz * dz) < q[3]
        elif kind == DISC:
            dx, dy, dz = x - q[0], y - q[1], z - q[2]
            m = ((dx * dx + dy * dy) < q[3]) & (np.fabs(dz) < q[4])
        elif kind == CUBOID:
            m = (x > q[0]) & (x < q[3]) & (y > q[1]) & (y < q[4]) & (z > q[2]) & (z < q[5])
        elif kind == BAND:
            field = BAND_FIELDS[int(q[0])]
            if field == "r":
                f = np.sqrt((x * x + y * y) + z * z)
            elif field == "rxy":
                f = np.sqrt(x * x + y * y)
            else:
                f = (x, y, z)["xyz".index(field)]
            m = np.ones(len(p), dtype=bool)
            if q[3]:
                m &= f > q[1]
            if q[4]:
                m &= f < q[2]
        else:
            raise ValueError(f"unknown region kind {kind!r}")
    return ~m if neg else m


def region_mask(pos, clauses) -> np.ndarray:
    """Mask of the conjunction of ``clauses`` (none: every particle)."""
    m = np.ones(len(pos), dtype=bool)
    for c in clauses or ():
        m &= clause_mask(pos, c)
    return m


def packed(clauses):
    """(nclauses, kinds, negate, params) as pbx_profile_set_region takes them
    (ctypes int arrays and an (n,6) float64 array); the clause count is
    checked by the library."""
    clauses = list(clauses or ())
    n = len(clauses)
    kinds = (ctypes.c_int * max(n, 1))(*[int(c[0]) for c in clauses])
    neg = (ctypes.c_int * max(n, 1))(*[int(bool(c[1])) for c in clauses])
    params = np.zeros((max(n, 1), 6))
    for k, c in enumerate(clauses):
        params[k] = c[2]
    return n, kinds, neg, params
