"""RadiusAtSurfaceDensity on the host: the reference's calculate against the
fixture recorded from the reference itself (tests/golden/make_golden_rsd.py),
and the numpy restatement of the device algorithm (tests/_rsd_data.py)
against the same fixture — which shows the fixture's cases keep the margin
the device route's bit parity rests on.  No GPU.
"""
import dataclasses

import numpy as np
import pytest

import _rsd_data as rd
from pynbodyext.calculate import ConstantProperty, ParamView, PropertyBase
from pynbodyext.filters import Sphere
from pynbodyext.simcore import SimArray, SimSnap

FX = rd.fixture()
CASE_IDS = [c.name for c in FX.cases]


def snapshot(case, dtype=np.float64):
    return SimSnap({"pos": FX.pos(case.dataset).astype(dtype),
                    "mass": FX.mass(case.dataset, case.mscale).astype(dtype)}, units_map=rd.UNITS)


def prop_of(case, target=None):
    from pynbodyext.properties import RadiusAtSurfaceDensity

    return RadiusAtSurfaceDensity(case.target if target is None else target, mode=case.mode,
                                  r_key=case.r_key, eps=case.eps)


def test_import_paths_signature_and_defaults():
    from pynbodyext import properties
    from pynbodyext.properties import base
    from pynbodyext.properties.base import RadiusAtSurfaceDensity

    assert properties.RadiusAtSurfaceDensity is RadiusAtSurfaceDensity
    assert "RadiusAtSurfaceDensity" in base.__all__ and "RadiusAtSurfaceDensity" in properties.__all__
    assert issubclass(RadiusAtSurfaceDensity, PropertyBase)
    fields = dataclasses.fields(RadiusAtSurfaceDensity)
    assert [f.name for f in fields] == ["target", "parameter", "mode", "r_key", "eps"]
    assert fields[0].default is dataclasses.MISSING
    assert [f.default for f in fields[1:]] == ["mass", "shell", "rxy", 0.01]
    assert "target" in RadiusAtSurfaceDensity.dynamic_param_specs
    p = RadiusAtSurfaceDensity(2.5)
    assert (p.target, p.parameter, p.mode, p.r_key, p.eps) == (2.5, "mass", "shell", "rxy", 0.01)
    with pytest.raises(TypeError):
        RadiusAtSurfaceDensity()


@pytest.mark.parametrize("case", FX.cases, ids=CASE_IDS)
def test_host_calculate_equals_the_reference(case):
    sim = snapshot(case)
    calc = prop_of(case)
    if case.info[0]:
        with pytest.raises(ValueError, match="^Could not bracket target surface density$"):
            calc(sim, backend="host")
        return
    res = calc.run(sim, backend="host", perf_time=True)
    assert "RadiusAtSurfaceDensity.calculate" in res.perf
    assert np.array_equal(rd.bits(res.value), rd.bits(case.radius))
    assert res.value.units == sim["pos"].units and res.value.sim is sim and res.value.shape == ()


def test_host_sigma_equals_the_reference():
    from pynbodyext.properties import RadiusAtSurfaceDensity

    n = 0
    for ds, r_key, eps, radii, s_total, s_shell in FX.sigma_lists():
        xs, cum = FX.table(ds, r_key)
        for mode, want in (("total", s_total), ("shell", s_shell), ("anything else", s_shell)):
            got = [RadiusAtSurfaceDensity._sigma_at_radius(r, xs, cum, eps, mode) for r in radii]
            assert np.array_equal(rd.bits(got), rd.bits(want)), (ds, r_key, mode)
            n += len(got)
    assert n > 500


@pytest.mark.parametrize("case", FX.cases, ids=CASE_IDS)
def test_product_square_restatement_equals_the_reference(case):
    """The device algorithm in numpy: the fixture's bits, path and margin."""
    xs, cum = FX.table(case.dataset, case.r_key, case.mscale)
    got = rd.solve_product(xs, cum, case.eps, case.mode, case.target)
    what, dist, need = got.worst()
    print(f"{case.name}: worst margin {what}: {dist:.3e} (needs > {need:.3e})")
    assert got.margin_ok, (what, dist, need)
    assert got.info == case.info
    assert np.array_equal(rd.bits(got.radius), rd.bits(case.radius))


def test_restated_sigma_is_within_its_bound_of_the_reference():
    for ds, r_key, eps, radii, s_total, s_shell in FX.sigma_lists():
        xs, cum = FX.table(ds, r_key)
        for mode, want in (("total", s_total), ("shell", s_shell)):
            for r, ref in zip(radii, want):
                got, bound = rd.sigma_product(r, xs, cum, eps, mode)
                assert abs(got - ref) <= bound * abs(ref), (ds, r_key, mode, r)


def test_fixture_covers_the_listed_cases():
    cases = FX.cases
    assert {c.mode for c in cases} == {"total", "shell"} and {c.r_key for c in cases} == {"r", "rxy"}
    solved = [c for c in cases if c.info[0] == 0]
    assert any(c.info[0] == 1 for c in cases)
    assert {0, rd.NGRID - 2} <= {c.info[1] for c in solved}
    assert any(c.info[3] == 1 and c.info[2] < rd.ITERS for c in solved)
    full = [c for c in solved if c.info[3] == 0]
    assert full and all(c.info[2] == rd.ITERS for c in full)
    assert any(c.radius in FX.table(c.dataset, c.r_key)[0] for c in full)  # onto a particle radius
    for c in cases:
        assert 0.1 <= abs(c.target) <= 10.0
    # the sigma lists: r <= 0, a clamped shell, an empty shell, radii equal to a particle's
    xs, cum = FX.table("dyadic", "r")
    assert len(np.unique(xs)) < len(xs)  # tied radii (equal masses)
    assert len(np.unique(FX.mass("dyadic"))) == 1
    _, _, eps, radii, s_total, s_shell = next(t for t in FX.sigma_lists() if t[0] == "dyadic")
    assert np.any(radii <= 0) and np.all(s_shell[radii <= 0] == 0.0)
    assert np.any((radii > 0) & (radii < 0.5 * eps))
    gap = radii == 301.0 / 64.0
    assert gap.any() and np.all(s_shell[gap] == 0.0) and np.all(s_total[gap] > 0.0)
    assert np.isin(radii, xs).sum() >= 6
    assert np.isin(radii - 0.5 * eps, xs).sum() >= 3 and np.isin(radii + 0.5 * eps, xs).sum() >= 3


def test_dynamic_and_unit_targets():
    case = next(c for c in FX.cases if c.name == "plummer_total_r")
    sim = snapshot(case)
    for target in (ConstantProperty(case.target), lambda s: case.target, "Msol kpc**-2",
                   np.array(case.target), SimArray([case.target], "Msol kpc**-2")):
        got = prop_of(case, target)(sim, backend="host")
        assert np.array_equal(rd.bits(got), rd.bits(case.radius))
    with pytest.raises(ValueError):  # (a mass is no surface density)
        prop_of(case, "Msol")(sim, backend="host")


def test_error_messages():
    case = next(c for c in FX.cases if c.name == "plummer_total_r")
    sim = snapshot(case)
    nothing = Sphere(1.0, cen=(500.0, 0.0, 0.0))
    with pytest.raises(IndexError, match="^index 0 is out of bounds for axis 0 with size 0$"):
        prop_of(case).filter(nothing)(sim, backend="host")
    one = SimSnap({"pos": np.array([[1.0, 2.0, 3.0]]), "mass": np.array([1.0])}, units_map=rd.UNITS)
    with pytest.raises(ValueError, match="^Degenerate radius distribution$"):
        prop_of(case)(one, backend="host")
    ring = SimSnap({"pos": np.array([[3.0, 4.0, 0.0], [-3.0, 4.0, 1.0], [5.0, 0.0, -2.0]]),
                    "mass": np.ones(3)}, units_map=rd.UNITS)
    from pynbodyext.properties import RadiusAtSurfaceDensity

    with pytest.raises(ValueError, match="^Degenerate radius distribution$"):
        RadiusAtSurfaceDensity(1.0, r_key="rxy")(ring, backend="host")
    with pytest.raises(ValueError, match="^Could not bracket target surface density$"):
        prop_of(case, 1e9)(sim, backend="host")


def test_in_sim_units():
    case = FX.cases[0]
    sim = snapshot(case)
    p = prop_of(case)
    assert p._in_sim_units(3, "mass", sim) == 3.0 and isinstance(p._in_sim_units(3, "mass", sim), float)
    assert p._in_sim_units(2.5, "mass", sim) == 2.5
    assert p._in_sim_units(np.float64(2.5), "mass", sim) == 2.5
    assert p._in_sim_units(np.array(4.0), "mass", sim) == 4.0  # a 0-d array
    assert p._in_sim_units(np.array([4.0]), "mass", sim) == 4.0
    assert p._in_sim_units(SimArray([2.0], "Msol"), "mass", sim) == 2.0
    assert p._in_sim_units(SimArray([2.0], "kpc"), "mass", sim, target_units="kpc") == 2.0
    assert p._in_sim_units("Msol", "mass", sim) == 1.0
    assert p._in_sim_units("kpc", "mass", sim, target_units="kpc") == 1.0
    with pytest.raises(TypeError, match="value must be scalar-like, got shape \\(2,\\)"):
        p._in_sim_units(np.array([1.0, 2.0]), "mass", sim)
    with pytest.raises(TypeError, match="unsupported value type"):
        p._in_sim_units(None, "mass", sim)
    with pytest.raises(TypeError, match="unsupported value type"):
        p._in_sim_units(np.int64(3), "mass", sim)  # (the reference accepts int and float only)


def test_device_plan_gate():
    """Which inputs get a device plan (none is run here: no GPU is touched)."""
    from pynbodyext.properties import RadiusAtSurfaceDensity

    case = next(c for c in FX.cases if c.name == "plummer_total_r")
    sim = snapshot(case)

    def plan(source, **kw):
        p = RadiusAtSurfaceDensity(**{"target": 1.0, **kw})
        values = {f.name: getattr(p, f.name) for f in dataclasses.fields(p)}
        return p.device_plan(source, {}, ParamView(values))

    assert callable(plan(sim)) and callable(plan(sim, r_key="r", mode="total"))
    assert plan(sim, r_key="x") is None and plan(sim, parameter="vr") is None
    for eps in (0.0, -0.01, np.inf, np.nan):
        assert plan(sim, eps=eps) is None
    for target in (np.inf, -np.inf, np.nan):
        assert plan(sim, target=target) is None
    assert plan(snapshot(case, np.float32)) is None  # float32 snapshots
    assert plan(sim[:]) is None  # sub-snapshots
