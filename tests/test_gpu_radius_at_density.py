"""RadiusAtSurfaceDensity on the device (csrc/profile.hip: cum_table,
cum_sigma_kernel, cum_solve_kernel).

The table against np.argsort(kind="stable") / np.cumsum bit for bit; sigma
against the product-square restatement of tests/_rsd_data.py bit for bit and
against the reference's recorded values within the propagated ulp of a
squared radius; the solve and the public property against every case of the
fixture recorded from the reference (tests/golden/make_golden_rsd.py), bits
and path; the public routes behind filters and a transform against the host
route on inputs whose margin the test recomputes first.
"""
import ctypes
import functools

import numpy as np
import pytest

import _rsd_data as rd
from pynbodyext import _native as nat
from pynbodyext.filters import Disc, FamilyFilter, Sphere
from pynbodyext.frame import unframe
from pynbodyext.profiles._device import SRC_W, DeviceBins
from pynbodyext.properties import RadiusAtSurfaceDensity
from pynbodyext.simcore import SimSnap
from pynbodyext.transforms import ShiftPosTo

pytestmark = pytest.mark.gpu

FX = rd.fixture()
CASE_IDS = [c.name for c in FX.cases]
FAMILIES = {"dm": slice(0, 2000), "star": slice(2000, 3000)}

# 2048: the LDS chunk of the sequential sum; 70001: past a radix tile
SIZES = [1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097, 70001]


# ------------------------------------------------------------------ 1. table
@functools.lru_cache(maxsize=None)
def cloud(n):
    rng = np.random.default_rng(9000 + n)
    return rng.normal(size=(n, 3)) * 3.0, rng.uniform(0.5, 1.5, n)


def check_table(d, x, w, built):
    order = np.argsort(x, kind="stable")
    xs, cum = d.cum_table()
    assert np.array_equal(rd.bits(xs), rd.bits(x[order]))
    assert np.array_equal(rd.bits(cum), rd.bits(np.cumsum(w[order])))
    assert np.array_equal(rd.bits(built), rd.bits([xs[0], xs[-1], cum[-1]]))


@pytest.mark.parametrize("route", ["set_x", "select"])
@pytest.mark.parametrize("n", SIZES)
def test_table(gpu, n, route):
    pos, w = cloud(n)
    if route == "set_x":
        x = pos[:, 0] * pos[:, 0] + 0.25  # (positive, unsorted)
        d = DeviceBins.from_x(x)
        built = d.cum_build(weights=w)
    else:
        x = rd.radii(pos, "r")
        d = DeviceBins.select(pos, w, ndim=3)
        assert d.n == n
        built = d.cum_build(weights=SRC_W)
    try:
        check_table(d, x, w, built)
    finally:
        d.close()


def test_table_ties_keep_index_order(gpu):
    """x quantised to 1/64 with distinct masses: only the stable order gives these sums."""
    pos, w = cloud(4097)
    x = np.round(np.abs(pos[:, 1]) * 64.0) / 64.0
    assert len(np.unique(x)) < len(x) // 4
    # (another tie order: equal x by descending index)
    other = np.cumsum(w[np.lexsort((-np.arange(len(x)), x))])
    assert not np.array_equal(other, np.cumsum(w[np.argsort(x, kind="stable")]))
    d = DeviceBins.from_x(x)
    try:
        check_table(d, x, w, d.cum_build(weights=w))
        assert not np.array_equal(d.cum_table()[1], other)
    finally:
        d.close()


def test_table_negative_x(gpu):
    pos, w = cloud(2049)
    x = pos[:, 2].copy()
    assert (x < 0).sum() > 500
    d = DeviceBins.from_x(x)
    try:
        check_table(d, x, w, d.cum_build(weights=w))
    finally:
        d.close()


def test_table_through_a_selection_with_a_scope(gpu):
    pos, w = cloud(70001)
    d = DeviceBins.select(pos, w, sphere=((0.5, 0.0, -0.5), 4.0), families=[(100, 60000)], ndim=2)
    try:
        idx, x, ws = d.selection()
        assert 1000 < d.n < 60000 and np.all(idx >= 100)
        check_table(d, x, ws, d.cum_build())
    finally:
        d.close()


# ------------------------------------------------------------------ 2. sigma
@functools.lru_cache(maxsize=None)
def handle(ds, r_key, mscale=1.0):
    """The fixture dataset's table on the device (kept for the module)."""
    d = DeviceBins.select(FX.pos(ds), FX.mass(ds, mscale), ndim=3 if r_key == "r" else 2)
    d.cum_build()
    return d


@pytest.mark.parametrize("mode", ["total", "shell"])
def test_sigma(gpu, mode):
    for ds, r_key, eps, radii, s_total, s_shell in FX.sigma_lists():
        xs, cum = FX.table(ds, r_key)
        d = handle(ds, r_key)
        got = d.cum_sigma(radii, mode=mode, eps=eps)
        mine = [rd.sigma_product(r, xs, cum, eps, mode) for r in radii]
        assert np.array_equal(rd.bits(got), rd.bits([s for s, _ in mine])), (ds, r_key)
        ref = s_total if mode == "total" else s_shell
        bound = np.array([b for _, b in mine])
        if mode == "total":
            assert np.all(bound <= 3 * rd.ULP)
        err = np.abs(got - ref)
        print(f"{ds}/{r_key} {mode}: max |device - reference| / bound = "
              f"{np.max(np.where(ref != 0, err / np.maximum(bound * np.abs(ref), 1e-300), 0.0)):.3f}, "
              f"{int((err != 0).sum())} of {len(ref)} differ")
        assert np.all(err <= bound * np.abs(ref)), (ds, r_key)


def test_sigma_mode_strings_and_single_radius(gpu):
    d = handle("plummer", "r")
    r = np.array([2.0])
    shell = d.cum_sigma(r, mode="shell", eps=0.5)
    assert np.array_equal(d.cum_sigma(2.0, mode="anything else", eps=0.5), shell)
    assert np.array_equal(d.cum_sigma(r, mode=0, eps=0.5), shell)
    assert np.array_equal(d.cum_sigma(r, mode=1), d.cum_sigma(r, mode="total"))
    grid = np.linspace(0.0, 12.0, 4096)  # the most one call takes
    xs, cum = FX.table("plummer", "r")
    want = [rd.sigma_product(x, xs, cum, 0.5, "shell")[0] for x in grid]
    assert np.array_equal(rd.bits(d.cum_sigma(grid, mode="shell", eps=0.5)), rd.bits(want))


# ------------------------------------------------------------------ 3. solve
@pytest.mark.parametrize("case", FX.cases, ids=CASE_IDS)
def test_solve(gpu, case):
    d = handle(case.dataset, case.r_key, case.mscale)
    xs, cum = FX.table(case.dataset, case.r_key, case.mscale)
    grid = np.linspace(max(xs[0], case.eps), xs[-1], rd.NGRID)
    radius, info = d.cum_solve(case.target, grid, mode=case.mode, eps=case.eps)
    assert list(info) == case.info
    assert np.array_equal(rd.bits(radius), rd.bits(case.radius))


def snapshot(case, dtype=np.float64, families=None):
    return SimSnap({"pos": FX.pos(case.dataset).astype(dtype),
                    "mass": FX.mass(case.dataset, case.mscale).astype(dtype)}, families=families,
                   units_map=rd.UNITS)


def prop_of(case, **kw):
    return RadiusAtSurfaceDensity(**{"target": case.target, "mode": case.mode,
                                     "r_key": case.r_key, "eps": case.eps, **kw})


@pytest.mark.parametrize("case", FX.cases, ids=CASE_IDS)
def test_public_property(gpu, case):
    sim = snapshot(case)
    if case.info[0]:
        with pytest.raises(ValueError, match="^Could not bracket target surface density$"):
            prop_of(case)(sim)
        return
    res = prop_of(case).run(sim, perf_time=True)
    assert "RadiusAtSurfaceDensity.device" in res.perf
    assert "RadiusAtSurfaceDensity.calculate" not in res.perf
    assert np.array_equal(rd.bits(res.value), rd.bits(case.radius))
    assert res.value.units == sim["pos"].units and res.value.sim is sim and res.value.shape == ()


# ----------------------------------------------------------- 4. public routes
def case_named(name):
    return next(c for c in FX.cases if c.name == name)


def check_against_host(calc, sim, host_view, r_key, mode, eps, target):
    """The device route's value equals the host route's on ``host_view`` (the
    particles the scope keeps, in the scope's frame) — after the margin of
    every decision on exactly that input has been recomputed and asserted."""
    xs, cum = rd.table(np.asarray(host_view[r_key]), np.asarray(host_view["mass"]))
    mine = rd.solve_product(xs, cum, eps, mode, target)
    what, dist, need = mine.worst()
    print(f"n={len(xs)} info={mine.info} worst margin {what}: {dist:.3e} (needs > {need:.3e})")
    assert mine.status == 0 and mine.margin_ok, (what, dist, need)
    res = calc.run(sim, perf_time=True)
    assert "RadiusAtSurfaceDensity.device" in res.perf
    assert "RadiusAtSurfaceDensity.calculate" not in res.perf
    host = RadiusAtSurfaceDensity(target, mode=mode, r_key=r_key, eps=eps)(host_view, backend="host")
    assert np.array_equal(rd.bits(res.value), rd.bits(mine.radius))
    assert np.array_equal(rd.bits(res.value), rd.bits(host))
    # .sim as ParamContain sets it: the snapshot, or the frame view of it a transform leads to
    assert res.value.units == host.units and unframe(res.value.sim)[0] is sim
    assert type(res.value.sim) is type(host.sim)
    return res


def test_behind_sphere_and_family(gpu):
    sim = snapshot(case_named("plummer_total_r"), families=FAMILIES)
    scope = Sphere(8.0) & FamilyFilter("dm")
    calc = RadiusAtSurfaceDensity(1.0, mode="total", r_key="r").filter(scope)
    view = sim[scope(sim)]
    assert 1500 < len(view) < 2000
    check_against_host(calc, sim, view, "r", "total", 0.01, 1.0)


def test_behind_a_disc_region(gpu):
    sim = snapshot(case_named("plummer_shell_rxy"), families=FAMILIES)
    scope = Disc(10.0, 2.0)
    calc = RadiusAtSurfaceDensity(0.5, mode="shell", r_key="rxy", eps=0.5).filter(scope)
    view = sim[scope(sim)]
    assert 1000 < len(view) < 3000
    check_against_host(calc, sim, view, "rxy", "shell", 0.5, 0.5)


def test_behind_a_transform(gpu):
    sim = snapshot(case_named("plummer_total_rxy"), families=FAMILIES)
    shift = ShiftPosTo("com")
    view = shift(sim)  # the snapshot in the frame the device route reads it in
    assert np.any(np.asarray(view["pos"]) != np.asarray(sim["pos"]))
    calc = RadiusAtSurfaceDensity(1.25, mode="total", r_key="rxy").transform(shift)
    check_against_host(calc, sim, view, "rxy", "total", 0.01, 1.25)
    assert np.array_equal(np.asarray(sim["pos"]), FX.pos("plummer"))  # (reverted: never touched)


def test_as_a_dynamic_parameter(gpu):
    """Sphere(RadiusAtSurfaceDensity(...)) sizes the aperture like the number written in."""
    from pynbodyext.properties import ParamSum

    case = case_named("plummer_total_r")
    sim = snapshot(case)
    inside = ParamSum("mass").filter(Sphere(prop_of(case)))(sim)
    number = ParamSum("mass").filter(Sphere(case.radius))(sim)
    assert float(inside) == float(number) > 0.0


@pytest.mark.parametrize("what", ["float32", "subsnap", "x", "parameter"])
def test_other_inputs_take_the_host_route(gpu, what):
    case = case_named("plummer_total_r")
    sim = snapshot(case, np.float32 if what == "float32" else np.float64)
    if what == "subsnap":
        sim = sim[:]
    calc = prop_of(case, **({"r_key": "x", "target": 30.0} if what == "x" else {}))
    if what == "parameter":
        sim["weight"] = np.asarray(sim["mass"])
        calc = prop_of(case, parameter="weight")
    res = calc.run(sim, perf_time=True)
    assert "RadiusAtSurfaceDensity.device" not in res.perf
    assert "RadiusAtSurfaceDensity.calculate" in res.perf
    if what in ("subsnap", "parameter"):
        assert np.array_equal(rd.bits(res.value), rd.bits(case.radius))


# ------------------------------------------------------------------ 5. errors
def test_public_errors(gpu):
    case = case_named("plummer_total_r")
    sim = snapshot(case)
    r = np.sort(rd.radii(FX.pos("plummer"), "r"))
    with pytest.raises(IndexError, match="^index 0 is out of bounds for axis 0 with size 0$"):
        prop_of(case).filter(Sphere(1.0, cen=(500.0, 0.0, 0.0)))(sim)
    with pytest.raises(ValueError, match="^Degenerate radius distribution$"):
        prop_of(case).filter(Sphere(0.5 * (r[0] + r[1])))(sim)  # one particle
    ring = SimSnap({"pos": np.array([[3.0, 4.0, 0.0], [-3.0, 4.0, 1.0], [5.0, 0.0, -2.0]]),
                    "mass": np.ones(3)}, units_map=rd.UNITS)
    res = None
    with pytest.raises(ValueError, match="^Degenerate radius distribution$"):
        res = RadiusAtSurfaceDensity(1.0, r_key="rxy").run(ring, perf_time=True)  # all radii equal
    assert res is None
    with pytest.raises(ValueError, match="^Could not bracket target surface density$"):
        prop_of(case, target=1e9)(sim)


def raises_value(call, *args):
    status = getattr(nat.load(), call)(*args)
    assert status == nat.PBX_ERR_VALUE, (call, status)
    return nat.last_error()


def test_library_errors(gpu):
    pos, w = cloud(257)
    d = DeviceBins.select(pos, w, ndim=3)
    try:
        h = d._h
        r = np.linspace(0.1, 5.0, 4097)
        out = np.empty(4097)
        info = np.zeros(4, dtype=np.int64)
        rad, lo, hi, tot = (ctypes.c_double() for _ in range(4))
        dp, i64 = nat.dptr, lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        # no table yet
        assert "pbx_profile_cum_build" in raises_value("pbx_profile_cum_sigma", h, 0, 0.01, 4, dp(r), dp(out))
        raises_value("pbx_profile_cum_get", h, dp(out), dp(out))
        raises_value("pbx_profile_cum_solve", h, 0, 0.01, 1.0, 256, dp(r), ctypes.byref(rad), i64(info))
        # bad arguments of the build
        raises_value("pbx_profile_cum_build", h, 0, None, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(tot))
        raises_value("pbx_profile_cum_build", h, 1, None, None, ctypes.byref(hi), ctypes.byref(tot))
        raises_value("pbx_profile_cum_build", h, 2, None, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(tot))
        d.cum_build()
        assert d.cum_sigma(r[:4096]).shape == (4096,)
        # counts, mode, null arguments
        assert "radii" in raises_value("pbx_profile_cum_sigma", h, 0, 0.01, 0, dp(r), dp(out))
        assert "radii" in raises_value("pbx_profile_cum_sigma", h, 0, 0.01, 4097, dp(r), dp(out))
        assert "mode" in raises_value("pbx_profile_cum_sigma", h, 2, 0.01, 4, dp(r), dp(out))
        assert "mode" in raises_value("pbx_profile_cum_sigma", h, -1, 0.01, 4, dp(r), dp(out))
        assert "null" in raises_value("pbx_profile_cum_sigma", h, 0, 0.01, 4, dp(r), None)
        assert "null" in raises_value("pbx_profile_cum_sigma", h, 0, 0.01, 4, None, dp(out))
        assert "null" in raises_value("pbx_profile_cum_get", h, dp(out), None)
        raises_value("pbx_profile_cum_solve", h, 0, 0.01, 1.0, 1, dp(r), ctypes.byref(rad), i64(info))
        raises_value("pbx_profile_cum_solve", h, 0, 0.01, 1.0, 4097, dp(r), ctypes.byref(rad), i64(info))
        raises_value("pbx_profile_cum_solve", h, 2, 0.01, 1.0, 256, dp(r), ctypes.byref(rad), i64(info))
        raises_value("pbx_profile_cum_solve", h, 0, 0.01, 1.0, 256, dp(r), None, i64(info))
        raises_value("pbx_profile_cum_solve", h, 0, 0.01, 1.0, 256, dp(r), ctypes.byref(rad), None)
        raises_value("pbx_profile_cum_solve", h, 0, 0.01, 1.0, 256, None, ctypes.byref(rad), i64(info))
        with pytest.raises(ValueError, match="mode"):
            d.cum_sigma(r[:4], mode=2)
        # whatever replaces x drops the table: no stale read
        DeviceBins.select(pos, w, sphere=((0.0, 0.0, 0.0), 2.0), ndim=3, into=d)
        with pytest.raises(ValueError, match="pbx_profile_cum_build"):
            d.cum_sigma(r[:4])
        d.cum_build()
        d.set_x(np.arange(5.0))
        with pytest.raises(ValueError, match="pbx_profile_cum_build"):
            d.cum_table()
        with pytest.raises(ValueError, match="no selection weights"):
            d.cum_build()  # (a set_x handle has none)
        d.cum_build(weights=np.ones(5))
        d.set_region([])
        d.cum_sigma(r[:4])  # (clearing no region changes nothing)
        empty = DeviceBins.select(pos, w, sphere=((90.0, 0.0, 0.0), 1.0), ndim=3)
        assert empty.n == 0
        with pytest.raises(ValueError, match="index 0 is out of bounds"):
            empty.cum_build()
        empty.close()
    finally:
        d.close()


def test_radial_equaln_drops_the_table(gpu):
    pos, w = cloud(4097)
    d = DeviceBins.select(pos, w, ndim=3)
    try:
        d.cum_build()
        DeviceBins.radial_equaln(pos, w, nbins=8, ndim=3, into=d)
        with pytest.raises(ValueError, match="pbx_profile_cum_build"):
            d.cum_table()
    finally:
        d.close()


# ------------------------------------------------------------- 6. determinism
def test_two_builds_and_solves_give_the_same_bits(gpu):
    case = case_named("plummer_shell_r")
    pos, mass = FX.pos(case.dataset), FX.mass(case.dataset, case.mscale)
    runs = []
    for _ in range(2):
        d = DeviceBins.select(pos, mass, ndim=3)
        try:
            lo, hi, tot = d.cum_build()
            xs, cum = d.cum_table()
            radius, info = d.cum_solve(case.target, np.linspace(max(lo, case.eps), hi, rd.NGRID),
                                       mode=case.mode, eps=case.eps)
            runs.append((rd.bits([lo, hi, tot, radius]), rd.bits(xs), rd.bits(cum), info))
        finally:
            d.close()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
