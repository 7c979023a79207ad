"""The filters on the host route (no GPU): masks against hand-written
expectations on crafted boundary particles, the composite identities, the
behaviours of the reference's filter tests, ``volume()``, what each filter
tells the device (``device_spec``), and the density properties against a
direct numpy sum.  The device passes are covered by tests/test_gpu_filters.py.
"""
import numpy as np
import pytest

import _filters_data as fd
from pynbodyext import filters
from pynbodyext import region as rg
from pynbodyext.calculate import and_specs
from pynbodyext.filters import (Annulus, BandPass, Cuboid, Disc, FamilyFilter, FilterBase, HighPass,
                                LowPass, SolarNeighborhood, Sphere)
from pynbodyext.properties import SurfaceDensity, VolumeDensity
from pynbodyext.simcore import SimSnap, as_unit, filt

UNITS = {"pos": "kpc", "vel": "km s**-1", "mass": "Msol"}


def crafted_snap():
    n = fd.NC
    return SimSnap({"pos": fd.CRAFTED.copy(), "vel": np.zeros((n, 3)), "mass": np.ones(n)},
                   families={"dm": slice(0, 4), "star": slice(4, n)}, units_map=UNITS)


@pytest.fixture(scope="module")
def snap():
    """x uniform in [0, 10): the reference's filter tests split it at 5 and 6."""
    rng = np.random.default_rng(11)
    n = 4000
    pos = rng.uniform(0.0, 10.0, size=(n, 3))
    pos[:, 1:] -= 5.0
    return SimSnap({"pos": pos, "vel": rng.normal(size=(n, 3)), "mass": rng.uniform(0.5, 1.5, n)},
                   families={"dm": slice(0, 1500), "gas": slice(1500, 2500), "star": slice(2500, n)},
                   units_map=UNITS)


def test_exports():
    for name in ("Sphere", "FamilyFilter", "Cuboid", "Disc", "Annulus", "BandPass", "HighPass",
                 "LowPass", "SolarNeighborhood"):  # the reference's filters.__all__
        assert name in filters.__all__ and issubclass(getattr(filters, name), FilterBase)
        assert hasattr(filt, name)
    assert rg.REGION_MAX == 8


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("name", sorted(fd.CASES))
def test_mask_on_crafted_particles(name):
    sim = crafted_snap()
    f, kept = fd.CASES[name]
    got = f(sim)
    assert got.dtype == bool
    assert set(np.flatnonzero(got)) == kept, name
    # the host mask is the region restatement the device tests compare against
    spec = f.device_spec(sim)
    assert spec is not None and "families" not in spec
    assert np.array_equal(rg.region_mask(fd.CRAFTED, fd.clauses_of(spec)), got)


def test_nan_and_infinity_under_plain_and_negated_clauses():
    sim = crafted_snap()
    odd = [9, 10, 11, 12]
    for name in ("sphere", "disc", "cuboid", "band_r", "band_rxy"):
        f = fd.CASES[name][0]
        assert not f(sim)[odd].any(), name
        assert (~f)(sim)[odd].all(), name
    # an open band keeps the infinity on its side, never a NaN
    assert HighPass("x", 0)(sim)[10] and not HighPass("x", 0)(sim)[9]
    assert LowPass("z", 0)(sim)[11] and not LowPass("z", 0)(sim)[12]
    assert (~LowPass("z", 0))(sim)[12]


def test_composites_are_their_definitions():
    sim = crafted_snap()
    assert np.array_equal(Annulus(0.5, 1.5, fd.CEN)(sim),
                          (Sphere(1.5, fd.CEN) & ~Sphere(0.5, fd.CEN))(sim))
    assert np.array_equal(SolarNeighborhood(0.5, 1.5, 0.5, fd.CEN)(sim),
                          (Disc(1.5, 0.5, fd.CEN) & ~Disc(0.5, 0.5, fd.CEN))(sim))
    assert Annulus(0.5, 1.5, fd.CEN)(sim)[2]  # d^2 == r1^2: the inner boundary is kept
    assert not Annulus(0.5, 1.5, fd.CEN)(sim)[1]  # d^2 == r2^2: the outer one is not
    c = Cuboid(-1.0)
    assert c.clauses(sim) == [rg.cuboid_clause(-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)]
    s = SolarNeighborhood()
    assert (s.r1, s.r2, s.height, s.cen) == ("5 kpc", "10 kpc", "2 kpc", (0, 0, 0))
    r1, r2, h = (float(as_unit(v).ratio(as_unit("kpc"))) for v in ("5 kpc", "10 kpc", "2 kpc"))
    assert s.clauses(sim) == [rg.disc_clause((0, 0, 0), r2, h),
                              rg.disc_clause((0, 0, 0), r1, h, negate=True)]


def test_stand_ins_agree_with_the_filters():
    sim = crafted_snap()
    pairs = [(filt.Cuboid(-1.0, -2.0, -3.0, 1.0, 2.0, 3.0), "cuboid"), (filt.Cuboid(-1.0), "cube"),
             (filt.Disc(1.5, 0.5, fd.CEN), "disc"), (filt.Annulus(0.5, 1.5, fd.CEN), "annulus"),
             (filt.SolarNeighborhood(0.5, 1.5, 0.5, fd.CEN), "solar"),
             (filt.BandPass("r", 5, 10), "band_r"), (filt.HighPass("r", 5), "high_r"),
             (filt.LowPass("z", 0), "low_z"), (~filt.Disc(1.5, 0.5, fd.CEN), "not_disc")]
    for f, name in pairs:
        assert np.array_equal(f(sim), fd.expected_mask(name)), name


# ------------------------------------- the reference's filter tests, restated
def test_band_pass_partitions(snap):
    bp1, bp2 = BandPass("x", 0, 5), BandPass("x", 5, 10)
    hp, lp = HighPass("x", 6), LowPass("x", 6)
    n = len(snap)
    assert len(snap[bp1]) + len(snap[bp2]) == n
    assert len(snap[hp]) + len(snap[lp]) == n
    assert len(snap[bp1 & bp2]) == 0 and len(snap[bp1 | bp2]) == n
    assert len(snap[~bp1]) == len(snap[bp2]) and len(snap[~bp2]) == len(snap[bp1])
    assert len(snap[~hp]) == len(snap[lp])
    assert len(snap[lp & hp]) == 0 and len(snap[lp | hp]) == n


def test_band_pass_bounds_as_number_unit_string_and_callable(snap):
    a = BandPass("x", 0, 10)
    b = BandPass("x", 0, "0.01 Mpc")
    c = BandPass("x", 0, lambda sim: sim["x"].max() + 0.1)
    assert len(snap[a]) == len(snap[b]) == len(snap[c]) == len(snap)
    five = float(as_unit("5 kpc").ratio(as_unit("kpc")))
    assert BandPass("x", 0, "5 kpc").device_spec(snap) == {"region": [rg.band_clause("x", 0, five)]}


def test_family_combinations(snap):
    stars, gas = FamilyFilter("star"), FamilyFilter("gas")
    either, both, not_stars = stars | gas, stars & gas, ~stars
    assert np.all(both(snap) <= either(snap)) and not both(snap).any()
    assert not (not_stars(snap) & stars(snap)).any()
    assert len(snap[either]) == 2500


def test_filter_scoped_by_a_filter(snap):
    bound = BandPass("x", 0, 2).with_filter(FamilyFilter("star"))
    star = snap[FamilyFilter("star")]
    assert np.array_equal(bound(snap), BandPass("x", 0, 2)(star))


def test_band_pass_on_another_field_is_a_host_mask(snap):
    f = BandPass("mass", 0.75, 1.25)
    m = np.asarray(snap["mass"])
    assert np.array_equal(f(snap), (m > 0.75) & (m < 1.25))
    assert f.device_spec(snap) is None
    assert (f & Sphere(3.0)).device_spec(snap) is None
    vr = np.asarray(snap["vr"])
    assert np.array_equal(HighPass("vr", 0)(snap), vr > 0)


# ----------------------------------------------------------------- volume
def test_volumes(snap):
    assert Sphere(2.0).volume() == 4.0 / 3.0 * np.pi * 2.0 ** 3
    assert Disc(3.0, 0.5).volume() == 2 * np.pi * 3.0 ** 2 * 0.5
    assert Disc("3 kpc", "500 pc").volume(snap) == pytest.approx(2 * np.pi * 9.0 * 0.5, rel=1e-14)
    assert Annulus(1.0, 2.0).volume() == 4.0 / 3.0 * np.pi * (2.0 ** 3 - 1.0 ** 3)
    assert SolarNeighborhood().volume(snap) == pytest.approx(2 * np.pi * 2.0 * (100.0 - 25.0),
                                                             rel=1e-14)
    assert Cuboid(-1.0, -2.0, -3.0, 1.0, 2.0, 4.0).volume() == 2.0 * 4.0 * 7.0
    assert Cuboid(-1.5).volume() == 27.0  # (the corners the mask fills in)


# ------------------------------------------------------------ device_spec
def test_device_spec_of_each_filter(snap):
    assert Sphere(2.0, fd.CEN).device_spec(snap).keys() == {"sphere"}
    assert Disc(2.0, 1.0, fd.CEN).device_spec(snap) == {"region": [rg.disc_clause(fd.CEN, 2.0, 1.0)]}
    assert Annulus(1.0, 2.0).device_spec(snap) == {
        "region": [rg.sphere_clause((0, 0, 0), 2.0), rg.sphere_clause((0, 0, 0), 1.0, negate=True)]}
    assert HighPass("rxy", 3).device_spec(snap) == {"region": [rg.band_clause("rxy", 3, None)]}
    kind, neg, q = rg.band_clause("rxy", None, 4.0)
    assert (kind, neg, q) == (rg.BAND, False, (4.0, 0.0, 4.0, 0.0, 1.0, 0.0))


def test_device_spec_and(snap):
    spec = (Disc("30 kpc", "2 kpc") & FamilyFilter("star")).device_spec(snap)
    r, h = (float(as_unit(v).ratio(as_unit("kpc"))) for v in ("30 kpc", "2 kpc"))
    assert spec == {"region": [rg.disc_clause((0, 0, 0), r, h)], "families": [(2500, 4000)]}
    # the first Sphere keeps the sphere slot, the second becomes a clause
    spec = (Sphere(3.0) & Sphere(2.0, fd.CEN) & LowPass("z", 1)).device_spec(snap)
    assert spec["sphere"][1] == 3.0
    assert spec["region"] == [rg.sphere_clause(fd.CEN, 2.0), rg.band_clause("z", None, 1)]
    assert and_specs({}, {"region": [rg.band_clause("x", 0, 1)]}) == \
        {"region": [rg.band_clause("x", 0, 1)]}
    assert and_specs(None, {}) is None


def test_device_spec_not(snap):
    assert (~Sphere(2.0, fd.CEN)).device_spec(snap) == \
        {"region": [rg.sphere_clause(fd.CEN, 2.0, negate=True)]}
    assert (~Disc(2.0, 1.0)).device_spec(snap) == \
        {"region": [rg.disc_clause((0, 0, 0), 2.0, 1.0, negate=True)]}
    assert (~~Disc(2.0, 1.0)).device_spec(snap) == {"region": [rg.disc_clause((0, 0, 0), 2.0, 1.0)]}
    # two clauses, a family, or a sphere with a family: not a single clause
    assert (~Annulus(1.0, 2.0)).device_spec(snap) is None
    assert (~FamilyFilter("star")).device_spec(snap) is None
    assert (~(Sphere(2.0) & FamilyFilter("star"))).device_spec(snap) is None
    assert (Disc(2.0, 1.0) | Sphere(1.0)).device_spec(snap) is None


def test_device_spec_beyond_eight_clauses_is_the_host_route(snap):
    f = Sphere(9.0)
    for k in range(8):
        f = f & HighPass("x", -float(k + 1))
    assert len(f.device_spec(snap)["region"]) == 8  # (the Sphere has its own slot)
    g = f & LowPass("x", 20.0)
    assert g.device_spec(snap) is None
    x = np.asarray(snap["x"])
    assert np.array_equal(g(snap), Sphere(9.0)(snap) & (x > -1.0) & (x < 20.0))


# ------------------------------------------------- densities on the host route
def test_densities_on_the_host_route(snap):
    view = snap[:]  # (a sub-snapshot always runs calculate on the host)
    p, m = np.asarray(snap["pos"]), np.asarray(snap["mass"])
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r2 = (x * x + y * y) + z * z
    shell = (r2 < 10.0 * 10.0) & ~(r2 < 2.0 * 2.0)
    vol = VolumeDensity(10.0, rmin=2.0)(view)
    assert float(vol) == m[shell].sum() / (4.0 / 3.0 * np.pi * (10.0 ** 3 - 2.0 ** 3))
    assert vol.units == as_unit("Msol kpc**-3")
    rxy = np.sqrt(x * x + y * y)
    ring = (rxy > 2.0) & (rxy < 10.0)
    surf = SurfaceDensity(10.0, 2.0)(view)
    assert float(surf) == m[ring].sum() / (np.pi * (10.0 ** 2 - 2.0 ** 2))
    assert surf.units == as_unit("Msol kpc**-2")
    assert float(VolumeDensity("10 kpc", rmin="2 kpc")(view)) == pytest.approx(float(vol), rel=1e-12)
    # defaults: rmin = 0, the whole sphere / disc; another parameter is summed as asked
    assert float(VolumeDensity(5.0)(view)) == m[r2 < 25.0].sum() / (4.0 / 3.0 * np.pi * 125.0)
    ones = VolumeDensity(5.0, parameter="x").run(snap, backend="host").value
    assert float(ones) == x[r2 < 25.0].sum() / (4.0 / 3.0 * np.pi * 125.0)
    # behind a filter, on the host backend
    star = np.zeros(len(m), dtype=bool)
    star[2500:] = True
    got = SurfaceDensity(10.0, 2.0).filter(FamilyFilter("star")).run(snap, backend="host").value
    assert float(got) == m[ring & star].sum() / (np.pi * (10.0 ** 2 - 2.0 ** 2))
