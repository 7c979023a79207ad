"""Shared by tests/test_filters_cpu.py and tests/test_gpu_filters.py: crafted
particles on the boundaries of every region primitive, the masks expected of
them written out by hand, and the filters under test.  Test infrastructure only.

Every coordinate is a dyadic rational, so the differences, squares and sums
below are exact in float64 and "on the boundary" means equality to the bit.
"""
from __future__ import annotations

import numpy as np

from pynbodyext import region as rg
from pynbodyext.filters import (Annulus, BandPass, Cuboid, Disc, HighPass, LowPass,
                                SolarNeighborhood, Sphere)

NAN, INF = np.nan, np.inf
CEN = (0.5, -0.25, 0.125)

CRAFTED = np.array([
    [0.5, -0.25, 0.125],    # 0  the centre
    [2.0, -0.25, 0.125],    # 1  cen + (1.5, 0, 0): d^2 == 1.5^2
    [0.5, -0.25, 0.625],    # 2  cen + (0, 0, 0.5): |dz| == 0.5 and d^2 == 0.5^2
    [2.0, -0.25, 0.375],    # 3  cen + (1.5, 0, 0.25): dx^2 + dy^2 == 1.5^2
    [-1.0, 0.0, 0.0],       # 4  x == x1 of the cuboid
    [1.0, 0.0, 0.0],        # 5  x == x2 of the cuboid
    [0.75, 1.5, -2.5],      # 6  inside the cuboid only
    [3.0, 4.0, 0.0],        # 7  r == rxy == 5
    [6.0, 8.0, 0.0],        # 8  r == rxy == 10
    [NAN, 0.0, 0.0],        # 9
    [INF, 0.0, 0.0],        # 10
    [0.0, 0.0, -INF],       # 11
    [0.0, 0.0, NAN],        # 12
    [1.5, 0.25, 0.25],      # 13 cen + (1, 0.5, 0.125): inside the sphere and the disc
    [0.0, 0.0, 7.0],        # 14 r == 7, rxy == 0
    [0.0, 6.0, 100.0],      # 15 rxy == 6, r > 100
    [1.0, -0.25, 0.375],    # 16 cen + (0.5, 0, 0.25): dx^2 + dy^2 == 0.5^2, x == x2
])
NC = len(CRAFTED)

# name -> (filter, the crafted particles it keeps)
CASES = {
    "sphere": (Sphere(1.5, CEN), {0, 2, 5, 13, 16}),
    "disc": (Disc(1.5, 0.5, CEN), {0, 5, 13, 16}),
    "cuboid": (Cuboid(-1.0, -2.0, -3.0, 1.0, 2.0, 3.0), {0, 2, 6}),
    "cube": (Cuboid(-1.0), {0, 2}),
    "band_r": (BandPass("r", 5, 10), {14}),
    "band_rxy": (BandPass("rxy", 5, 10), {15}),
    "band_x": (BandPass("x", 0.5, 2.0), {5, 6, 13, 16}),
    "high_r": (HighPass("r", 5), {8, 10, 11, 14, 15}),
    "low_r": (LowPass("r", 5), {0, 1, 2, 3, 4, 5, 6, 13, 16}),
    "low_z": (LowPass("z", 0), {6, 11}),
    "annulus": (Annulus(0.5, 1.5, CEN), {2, 5, 13, 16}),
    "solar": (SolarNeighborhood(0.5, 1.5, 0.5, CEN), {5, 13, 16}),
}
# the negation of every single-clause case keeps the complement, NaN rows included
for _name in ("sphere", "disc", "cuboid", "band_r", "band_rxy", "high_r", "low_z"):
    _f, _kept = CASES[_name]
    CASES["not_" + _name] = (~_f, set(range(NC)) - _kept)
# five clauses: disc & ~small sphere & cuboid & x band & z band
CASES["and5"] = (Disc(1.5, 0.5, CEN) & ~Sphere(0.25, CEN) & Cuboid(-1.0, -2.0, -3.0, 1.5, 2.0, 3.0)
                 & HighPass("x", 0.5) & LowPass("z", 0.375), {5})


def expected_mask(name, n=NC):
    m = np.zeros(n, dtype=bool)
    m[list(CASES[name][1])] = True
    return m


def clauses_of(spec):
    """The clauses a device_spec amounts to, its sphere slot included (for the
    numpy oracle)."""
    out = list(spec.get("region") or ())
    if spec.get("sphere") is not None:
        out.append(rg.sphere_clause(*spec["sphere"]))
    return out
