"""VirialRadius and SpinParam on the host: the public surface, the snapshot's
``properties`` dict and the restatements of pynbody's routines in simcore
(DESIGN §6).  No GPU."""
import dataclasses
import math

import numpy as np
import pytest

import _halo_data as hd
from pynbodyext import properties, simcore
from pynbodyext.filters import FamilyFilter, Sphere
from pynbodyext.frame import Frame, FrameView
from pynbodyext.properties import generic
from pynbodyext.simcore import SimSnap, as_unit
from pynbodyext.transforms import ShiftPosTo, ShiftVelTo

N, SEED = 20000, 11


def sim():
    return hd.halo(N, SEED)


# ------------------------------------------------------------------ surface
def test_exports_fields_defaults():
    for name in ("VirialRadius", "SpinParam"):
        assert name in properties.__all__ and name in generic.__all__
        assert getattr(properties, name) is getattr(generic, name)
    vr = properties.VirialRadius()
    assert [(f.name, f.default) for f in dataclasses.fields(vr)] == \
        [("overdensity", 178.), ("rho_def", "critical")]
    assert properties.VirialRadius(200., "matter").rho_def == "matter"
    assert properties.VirialRadius(overdensity=200.).overdensity == 200.
    assert dataclasses.fields(properties.SpinParam()) == ()
    with pytest.raises(ValueError, match=r"Invalid rho_def: virial\. Expected one of "
                                         r"\['critical', 'matter'\]\."):
        properties.VirialRadius(rho_def="virial")
    # still excluded
    with pytest.raises(NotImplementedError):
        properties.CenPos("pot")


def test_snapshot_properties():
    s = sim()
    assert s.properties == hd.PROPERTIES and isinstance(s.properties, dict)
    assert s[::2].properties is s.properties
    assert s.dm[Sphere("50 kpc")(s.dm)].properties is s.properties
    view = FrameView(s, Frame(c=(1.0, 2.0, 3.0)))
    assert view.properties is s.properties
    assert view[:10].properties is s.properties
    assert Frame(c=(1.0, 2.0, 3.0)).apply(s).properties == hd.PROPERTIES
    bare = SimSnap({"pos": np.zeros((2, 3)), "mass": np.ones(2)})
    assert bare.properties == {}
    with pytest.raises(KeyError):
        bare.properties["h"]
    with pytest.raises(KeyError):  # the calculators read them
        properties.VirialRadius()(SimSnap({"pos": np.ones((2, 3)), "mass": np.ones(2)},
                                          units_map=hd.UNITS), backend="host")
    # a snapshot's dict is its own
    props = dict(hd.PROPERTIES)
    other = SimSnap({"pos": np.zeros((2, 3)), "mass": np.ones(2)}, properties=props)
    props["z"] = 9.0
    assert other.properties["z"] == hd.PROPERTIES["z"]


# --------------------------------------------------------------- cosmology
def test_rho_crit_closed_form():
    """3 H^2 / (8 pi G) at z = 0 is about 277.5 h^2 Msol kpc^-3; at z the
    closed form scales it by E(z)^2."""
    s = sim()
    h = hd.PROPERTIES["h"]
    rc0 = simcore.rho_crit(s, z=0)
    assert rc0 == pytest.approx(277.5 * h * h, rel=1e-3)
    # by hand from the package's constants, in SI
    si = {k: as_unit(k).scale for k in ("km", "Mpc", "Msol", "kpc", "G")}
    h0 = 100.0 * h * si["km"] / si["Mpc"]
    by_hand = 3.0 * h0 * h0 / (8.0 * math.pi * si["G"]) / (si["Msol"] / si["kpc"] ** 3)
    assert rc0 == pytest.approx(by_hand, rel=1e-12)
    z = hd.PROPERTIES["z"]
    e2 = 0.3 * (1 + z) ** 3 + 0.7
    assert simcore.rho_crit(s) == pytest.approx(rc0 * e2, rel=1e-12)
    assert simcore.rho_crit(s, z=z) == simcore.rho_crit(s)
    # other units of the snapshot
    s2 = SimSnap({"pos": np.ones((1, 3)), "mass": np.ones(1)},
                 units_map={"pos": "Mpc", "mass": "1e10 Msol"}, properties=hd.PROPERTIES)
    assert simcore.rho_crit(s2, z=0) == pytest.approx(rc0 * 1e9 / 1e10, rel=1e-12)
    # the two reference densities
    assert simcore.virial_target_density(s, 200.0, "critical") == \
        pytest.approx(200.0 * rc0 * e2, rel=1e-12)
    assert simcore.virial_target_density(s, 200.0, "matter") == \
        pytest.approx(200.0 * 0.3 * rc0 * (1 + z) ** 3, rel=1e-12)


# ------------------------------------------------------------ VirialRadius
@pytest.mark.parametrize("rho_def", ["critical", "matter"])
@pytest.mark.parametrize("overdensity", [178.0, 2000.0])
def test_virial_radius_independent_check(overdensity, rho_def):
    s = sim()
    r = properties.VirialRadius(overdensity, rho_def)(s, backend="host")
    assert isinstance(r, float) and r > 0
    target = simcore.virial_target_density(s, overdensity, rho_def)
    pos, mass = np.asarray(s["pos"]), np.asarray(s["mass"])
    inside = np.sqrt((pos ** 2).sum(axis=1)) < r
    rho = mass[inside].sum() / (4.0 / 3.0 * math.pi * r ** 3)
    print(f"overdensity {overdensity} {rho_def}: r = {r:.6f}, |target - rho| / target = "
          f"{abs(target - rho) / target:.3e}")
    assert abs(target - rho) < 1e-3 * target


def test_virial_cases_admitted():
    """Every case of the device test keeps its decisions clear of the
    boundaries (hd.virial_case asserts it) and converges in 6 to 18 steps."""
    its = [hd.virial_case(*case)[2] for case in hd.VIRIAL_CASES]
    assert len(its) == 18 and min(its) >= 6 and max(its) <= 18, its


def test_bisect_is_pynbodys_loop():
    calls = []

    def f(x):
        calls.append(x)
        return x - 0.3  # (z < 0 moves the left bound: the root of an increasing f)

    root, it = simcore.bisect_iterations(0.0, 1.0, f, 0.01)
    assert calls[:3] == [0.5, 0.25, 0.375] and it == len(calls) and abs(root - 0.3) < 0.01
    assert simcore.bisect_iterations(1.0, 0.0, f, 0.01) == (0.5, 0)  # right < left
    with pytest.raises(ValueError, match="Bisection algorithm did not converge"):
        simcore.bisect_iterations(0.0, 1.0, lambda x: 1.0, 0.01, niter_max=5)


def test_virial_radius_not_converged():
    s, overdensity = hd.three_particles()
    with pytest.raises(ValueError, match="Bisection algorithm did not converge"):
        properties.VirialRadius(overdensity)(s, backend="host")


def test_virial_radius_empty_scope():
    with pytest.raises(ValueError, match="zero-size array"):
        properties.VirialRadius().filter(Sphere(1e-9))(sim(), backend="host")


# --------------------------------------------------------------- SpinParam
def spin_by_hand(pos, vel, mass):
    g = float((simcore.units.G * as_unit("Msol") / as_unit("kpc")).ratio(as_unit("km s**-1") ** 2))
    m_tot = mass.sum()
    r_max = np.sqrt((pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]) + pos[:, 2] * pos[:, 2]).max()
    v = np.sqrt(g * m_tot / r_max)
    ang = (mass.reshape((len(mass), 1)) * np.cross(pos, vel)).sum(axis=0)
    j = np.sqrt((ang * ang).sum())
    return float(j / (np.sqrt(2.0) * m_tot * v * r_max))


def test_spin_param_formula():
    s = sim()
    pos, vel, mass = (np.asarray(s[k]) for k in ("pos", "vel", "mass"))
    lam = properties.SpinParam()(s, backend="host")
    assert isinstance(lam, float) and 0.0 < lam < 1.0
    assert lam == spin_by_hand(pos, vel, mass)
    # G in (km/s)^2 kpc / Msol
    g = float((simcore.units.G * as_unit("Msol") / as_unit("kpc")).ratio(as_unit("km s**-1") ** 2))
    assert g == pytest.approx(4.30091e-6, rel=1e-4)
    with pytest.raises(ValueError, match="zero-size array"):
        properties.SpinParam().filter(Sphere(1e-9))(s, backend="host")


# -------------------------------------------------------- scopes, arithmetic
def test_host_run_under_filter_and_transform():
    s = sim()
    pos, vel, mass = (np.asarray(s[k]) for k in ("pos", "vel", "mass"))
    shift, boost = np.array([30.0, -20.0, 10.0]), np.array([50.0, 10.0, -5.0])
    moved = hd.snapshot(pos + shift, vel + boost, mass)
    frame = ShiftPosTo("ssc").then(ShiftVelTo("com").filter(Sphere("5 kpc")))
    rvir = properties.VirialRadius(overdensity=200.).transform(frame)(moved, backend="host")
    lam = properties.SpinParam().filter(Sphere(rvir)).transform(frame)(moved, backend="host")
    r0 = properties.VirialRadius(overdensity=200.)(s, backend="host")
    assert rvir == pytest.approx(r0, rel=2e-2)  # (the shrinking-sphere centre is not the origin)
    assert 0.0 < lam < 1.0
    # a filter scope: the dm particles only, written out by hand
    dm = s.family_slice("dm")
    sub = hd.snapshot(pos[dm], vel[dm], mass[dm])
    assert properties.VirialRadius(200.).filter(FamilyFilter("dm"))(s, backend="host") == \
        simcore.virial_radius(sub, 200.0)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    inside = ((x * x + y * y) + z * z) < 100.0 * 100.0
    assert properties.SpinParam().filter(Sphere(100.0))(s, backend="host") == \
        spin_by_hand(pos[inside], vel[inside], mass[inside])


def test_arithmetic_between_properties():
    s = sim()
    rv = properties.VirialRadius(200.)
    lam = properties.SpinParam()
    a, b = rv(s, backend="host"), lam(s, backend="host")
    assert (rv * lam)(s, backend="host") == a * b
    assert (rv / 2 + 1)(s, backend="host") == a / 2 + 1
    assert (1 - lam)(s, backend="host") == 1 - b
    assert (-rv)(s, backend="host") == -a
