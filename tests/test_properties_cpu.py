"""Property calculators on the host route (no GPU).

Every property is evaluated on a sub-snapshot view (``sim[:]``), which by
the routing rules of pynbodyext/properties/_device.py always runs the
reference's numpy ``calculate``; the checker is each formula written out
here.  The device route and the profile built behind
``Sphere(ParamContain(...))`` are covered by tests/test_gpu_properties.py
(building a profile needs the device).
"""
import numpy as np
import pytest

from pynbodyext import calculate
from pynbodyext.calculate import ConstantProperty, OpProperty, Param, PropertyBase
from pynbodyext.filters import FamilyFilter, Sphere
from pynbodyext.properties import (AngMomVec, CenPos, CenVel, KappaRot, KappaRotMean, ParamContain,
                                   ParameterContain, ParamSum, PatternSpeed)
from pynbodyext.properties import _device as pdev
from pynbodyext.simcore import SimArray, SimSnap, SubSnap, as_unit, shrink_sphere_center

UNITS = {"pos": "kpc", "vel": "km s**-1", "mass": "Msol"}


def make_snap(n=3000, seed=5, dtype=np.float64):
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(n, 3)) * np.array([3.0, 2.0, 1.0]) + np.array([0.3, -0.2, 0.1])
    vel = rng.normal(size=(n, 3))
    mass = rng.uniform(0.5, 1.5, n)
    return SimSnap({"pos": pos.astype(dtype), "vel": vel.astype(dtype), "mass": mass.astype(dtype)},
                   families={"dm": slice(0, 1800), "star": slice(1800, n)}, units_map=UNITS)


@pytest.fixture(scope="module")
def snap():
    root = make_snap()
    view = root[:]
    assert isinstance(view, SubSnap)
    return root, view


def arrays(root):
    p, v, m = (np.asarray(root[k]) for k in ("pos", "vel", "mass"))
    return p[:, 0], p[:, 1], p[:, 2], v[:, 0], v[:, 1], v[:, 2], m


def test_exports():
    assert ParameterContain is ParamContain
    for name in ("Param", "ParamView", "PropertyBase", "ConstantProperty", "OpProperty"):
        assert name in calculate.__all__
    assert pdev.NSUMS == 18 and pdev.ALL_GROUPS == 127


def test_derived_fields(snap):
    root, _ = snap
    x, y, z, vx, vy, vz, m = arrays(root)
    assert np.array_equal(root["vcxy"], (-y * vx + x * vy) / np.sqrt(x ** 2 + y ** 2))
    assert np.array_equal(root["vcxy"], root["vphi"])
    assert np.array_equal(root["ke"], 0.5 * ((vx * vx + vy * vy) + vz * vz))
    assert root["vcxy"].units == as_unit("km s**-1")
    assert root["ke"].units == as_unit("km**2 s**-2")


def test_param_sum(snap):
    root, view = snap
    got = ParamSum("mass").run(view, perf_time=True)
    assert "ParamSum.device" not in got.perf and "ParamSum.calculate" in got.perf
    assert got.value == np.asarray(root["mass"]).sum()
    assert got.value.units == as_unit("Msol")
    assert ParamSum("x")(view) == np.asarray(root["x"]).sum()


def test_centres(snap):
    root, view = snap
    x, y, z, vx, vy, vz, m = arrays(root)
    cen = CenPos("com")(view)
    assert np.array_equal(cen, (np.asarray(root["pos"]).T * m).sum(axis=1) / m.sum())
    assert cen.units == as_unit("kpc") and cen.sim is view
    assert np.array_equal(root.mean_by_mass("pos"), cen)
    cv = CenVel()(view)
    assert np.array_equal(cv, (np.asarray(root["vel"]).T * m).sum(axis=1) / m.sum())
    assert cv.units == as_unit("km s**-1") and cv.sim is view


def shrink_reference(pos, mass, r0=None, factor=0.7, min_particles=100):
    com = (pos.T * mass).sum(axis=1) / mass.sum()
    r = (pos[:, 0].max() - pos[:, 0].min()) / 2 if r0 is None else r0
    it = 0
    while True:
        d = pos - com
        keep = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < r * r
        if keep.sum() <= min_particles:
            return com, it
        com = (pos[keep].T * mass[keep]).sum(axis=1) / mass[keep].sum()
        r *= factor
        it += 1


def test_shrinking_sphere(snap):
    root, view = snap
    pos, mass = np.asarray(root["pos"]), np.asarray(root["mass"])
    ref, it = shrink_reference(pos, mass)
    assert it > 3
    cen = CenPos()(view)  # mode "ssc" is the default
    assert np.array_equal(cen, ref) and cen.units == as_unit("kpc") and cen.sim is view
    assert np.array_equal(shrink_sphere_center(root, r=2.5, shrink_factor=0.8, min_particles=50),
                          shrink_reference(pos, mass, 2.5, 0.8, 50)[0])
    few = root[np.arange(60)]  # n <= min_particles: the plain centre of mass
    assert np.array_equal(CenPos("ssc")(few), few.mean_by_mass("pos"))


def test_angular_momentum(snap):
    root, view = snap
    x, y, z, vx, vy, vz, m = arrays(root)
    L = AngMomVec()(view)
    ref = np.stack([m * (y * vz - z * vy), m * (z * vx - x * vz), m * (x * vy - y * vx)]).sum(axis=1)
    assert np.allclose(L, ref, rtol=1e-12, atol=0)
    assert np.array_equal(L, (m[:, None] * np.cross(np.asarray(root["pos"]), np.asarray(root["vel"]))).sum(axis=0))
    assert L.units == as_unit("Msol kpc km s**-1")


def test_kappa(snap):
    root, view = snap
    x, y, z, vx, vy, vz, m = arrays(root)
    vc = (x * vy - y * vx) / np.sqrt(x * x + y * y)
    ke = 0.5 * ((vx * vx + vy * vy) + vz * vz)
    k = KappaRot()(view)
    assert isinstance(k, float) and k == float(np.sum(0.5 * m * vc ** 2) / np.sum(m * ke))
    km = KappaRotMean()(view)
    assert isinstance(km, float) and km == float(np.mean(0.5 * vc ** 2 / ke))
    assert 0 < k < 1 and 0 < km < 1


def test_pattern_speed(snap):
    root, view = snap
    x, y, z, vx, vy, vz, m = arrays(root)
    Ixx, Iyy, Ixy = (m * x * x).sum(), (m * y * y).sum(), (m * x * y).sum()
    Im = 1 / 2 * (Ixx - Iyy)
    dIxy, dIm = (m * (x * vy + y * vx)).sum(), (m * (x * vx - y * vy)).sum()
    ref = 1 / 2 * (Im * dIxy - dIm * Ixy) / (Im * Im + Ixy * Ixy)
    w = PatternSpeed()(view)
    assert w == ref and w.units == as_unit("km s**-1 kpc**-1") and w.sim is root


def contain_reference(key, w, frac):
    order = np.argsort(key, kind="stable")
    ks, c = key[order], np.cumsum(w[order])
    return np.interp(np.atleast_1d(np.asarray(frac, dtype=float)), (c - c[0]) / (c[-1] - c[0]), ks)


def test_param_contain(snap):
    root, view = snap
    r, rxy, m = np.asarray(root["r"]), np.asarray(root["rxy"]), np.asarray(root["mass"])
    half = ParamContain()(view)
    assert half.shape == () and half == contain_reference(r, m, 0.5)[0]
    assert half.units == as_unit("kpc") and half.sim is root
    got = ParamContain(frac=[0.1, 0.5, 0.9], cal_key="rxy")(view)
    assert np.array_equal(got, contain_reference(rxy, m, [0.1, 0.5, 0.9]))
    # the field-first positional order, and the dataclass's own
    assert ParamContain("r", 0.5)(view) == half and ParamContain(0.5, "r")(view) == half
    p = ParamContain("rxy", 0.25)
    assert (p.frac, p.cal_key, p.parameter) == (0.25, "rxy", "mass")
    # dynamic fractions: a callable and another property
    assert ParamContain(frac=lambda s: 0.5)(view) == half
    assert ParamContain(frac=ConstantProperty(0.5))(view) == half


def test_error_texts(snap):
    root, view = snap
    with pytest.raises(ValueError, match=r"Invalid mode: nope. Expected one of \['ssc', 'com', 'pot', 'hyb'\]."):
        CenPos("nope")
    with pytest.raises(ValueError, match="Invalid mode: ssc. Expected 'com'."):
        CenVel("ssc")
    for mode in ("pot", "hyb"):
        with pytest.raises(NotImplementedError, match=mode):
            CenPos(mode)
    for bad in (0.0, 1.0, 1.5, [0.5, -0.1]):
        with pytest.raises(ValueError, match="frac values must be between 0 and 1, got"):
            ParamContain(frac=bad)(view)
    with pytest.raises(ValueError, match="frac must be a scalar or 1D sequence."):
        ParamContain(frac=[[0.5]])(view)
    zero = SimSnap({"pos": np.asarray(root["pos"])[:10], "mass": np.zeros(10)})[:]
    with pytest.raises(ValueError, match="Non-positive total 'mass'; cannot compute containment radius."):
        ParamContain()(zero)
    with pytest.raises(IndexError):
        ParamContain()(root[np.zeros(0, dtype=np.int64)])
    with pytest.raises(TypeError, match=r"PropertyBase is symbolic; evaluate with run\(\) or value\(\)."):
        bool(ParamContain())
    with pytest.raises(TypeError, match="symbolic"):
        if 2 * ParamContain():
            pass


def test_arithmetic(snap):
    root, view = snap
    half = ParamContain()(view)
    two = 2 * ParamContain()
    assert isinstance(two, OpProperty)
    assert two(view) == 2 * half
    assert (ParamContain() * 2)(view) == half * 2
    assert (ParamContain() + 1.5)(view) == half + 1.5 and (1.5 + ParamContain())(view) == 1.5 + half
    assert (ParamContain() - 1)(view) == half - 1 and (1 - ParamContain())(view) == 1 - half
    assert (ParamContain() / 4)(view) == half / 4 and (4 / ParamContain())(view) == 4 / half
    assert (-ParamContain())(view) == -half
    assert (ParamContain() / ParamSum("mass"))(view) == half / np.asarray(root["mass"]).sum()
    assert np.array_equal((CenPos("com") - CenPos("com"))(view), np.zeros(3))
    assert ConstantProperty(3.0)(view) == 3.0


def test_declarative_fields():
    @PropertyBase.dataclass
    class Scaled(PropertyBase):
        scale: Param[float] = Param(field_name="pos")
        offset: Param[float] = Param(default=0.0)
        key: str = "x"

        def calculate(self, sim, params=None):
            return params.scale * float(np.asarray(sim[params["key"]]).sum()) + params.offset

    assert Scaled.dynamic_param_specs == {"scale": "pos", "offset": None}
    with pytest.raises(TypeError):
        Scaled()  # scale has no default
    root = make_snap(50)
    s = float(np.asarray(root["x"]).sum())
    assert Scaled(2.0)(root[:]) == 2.0 * s
    assert Scaled("1 pc", offset=lambda sim: 1.0)(root[:]) == as_unit("pc").ratio("kpc") * s + 1.0
    assert Scaled(ConstantProperty(3.0), key="y")(root[:]) == 3.0 * float(np.asarray(root["y"]).sum())
    assert hash(Scaled(1.0)) != hash(Scaled(1.0))  # identity, like every calculator


def test_calculator_valued_sphere(snap):
    """Sphere(2 * ParamContain()) resolves to the number written in: the same
    mask and the same device description."""
    root, view = snap
    half = float(ParamContain()(view))
    for radius, number in ((ParamContain("r", 0.5), half), (2 * ParamContain(), 2 * half)):
        f, g = Sphere(radius), Sphere(number)
        assert np.array_equal(f(view), g(view)) and 0 < f(view).sum() < len(view)
        sf, sg = f.device_spec(view), g.device_spec(view)
        assert sf["sphere"][1] == sg["sphere"][1] == number
        assert np.array_equal(sf["sphere"][0], sg["sphere"][0])
    cen = CenPos("com")
    f = Sphere(1.0, cen=cen)
    assert np.array_equal(f(view), Sphere(1.0, cen=np.asarray(cen(view)))(view))


def test_bound_property_host_route(snap):
    """A property behind a filter on a view: mask first, then calculate."""
    root, view = snap
    filt = Sphere(2.0, cen=(0.3, -0.2, 0.1)) & FamilyFilter("star")
    mask = filt(view)
    res = CenPos("com").filter(filt).run(view, perf_time=True)
    assert "CenPos.device" not in res.perf
    sub = view[mask]
    assert np.array_equal(res.value, sub.mean_by_mass("pos"))
    assert KappaRot().filter(filt)(view) == KappaRot()(sub)


def test_float32_snapshot_takes_host_route():
    root = make_snap(500, dtype=np.float32)
    for prop in (ParamSum("mass"), CenPos("com"), ParamContain(), KappaRot()):
        res = prop.run(root, perf_time=True)
        assert f"{type(prop).__name__}.calculate" in res.perf
        assert f"{type(prop).__name__}.device" not in res.perf


def test_routing_conditions():
    root = make_snap(100)
    assert set(pdev.snapshot_arrays(root, ("pos", "vel", "mass"))) == {"pos", "vel", "mass"}
    assert pdev.snapshot_arrays(root[:], ("pos",)) is None  # a view
    assert pdev.snapshot_arrays(make_snap(100, dtype=np.float32), ("pos",)) is None
    user = make_snap(100)
    user["ke"] = np.ones(100)  # a user's own column: the host route reads it
    assert pdev.snapshot_arrays(user, ("pos", "vel", "mass")) is None
    assert KappaRot().run(user, perf_time=True).perf.keys() == {"KappaRot.calculate"}
    strided = SimSnap({"pos": np.zeros((100, 6))[:, ::2], "mass": np.ones(100)})
    assert pdev.snapshot_arrays(strided, ("pos", "mass")) is None
    # which properties have a device plan at all
    assert ParamSum("x").device_plan(root, {}, calculate.ParamView({"parameter": "x"})) is None
    pv = calculate.ParamView({"frac": 0.5, "cal_key": "x", "parameter": "mass"})
    assert ParamContain(cal_key="x").device_plan(root, {}, pv) is None
    sph = {"sphere": (np.zeros(3), 1.0)}
    assert CenPos("ssc").device_plan(root, sph, calculate.ParamView({"mode": "ssc"})) is None
    assert callable(CenPos("ssc").device_plan(root, {}, calculate.ParamView({"mode": "ssc"})))
