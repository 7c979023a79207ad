"""Kinematic fields of the snapshot layer (no GPU): vr, vtheta, vphi, vrxy, v2, vt.

The checker is the numpy restatement of the definitions the host
(pynbodyext.simcore.kinematic_field) and the device (csrc/profile.hip,
kin_fields) share: float64, these expressions in this order.
"""
import numpy as np
import pytest

from pynbodyext import _native
from pynbodyext.simcore import KINEMATIC_FIELDS, NoUnit, SimSnap, as_unit


def reference_fields(pos, vel):
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    vx, vy, vz = vel[:, 0], vel[:, 1], vel[:, 2]
    with np.errstate(all="ignore"):
        rxy2 = x * x + y * y
        r2 = rxy2 + z * z
        rxy = np.sqrt(rxy2)
        r = np.sqrt(r2)
        s = x * vx + y * vy
        vr = (s + z * vz) / r
        vrxy = s / rxy
        vphi = (x * vy - y * vx) / rxy
        vtheta = (z * vrxy - rxy * vz) / r
        v2 = (vx * vx + vy * vy) + vz * vz
        vt = np.sqrt(v2 - vr * vr)
    return {"vr": vr, "vtheta": vtheta, "vphi": vphi, "vrxy": vrxy, "v2": v2, "vt": vt}


def make_arrays(n=1000, seed=7):
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(n + 2, 3))
    vel = rng.normal(size=(n + 2, 3))
    pos[n] = 0.0                 # the origin
    pos[n + 1] = (0.0, 0.0, 1.5)  # on the z axis
    mass = rng.uniform(0.5, 1.5, n + 2)
    return pos, vel, mass


@pytest.fixture(scope="module")
def snap():
    pos, vel, mass = make_arrays()
    sim = SimSnap({"pos": pos, "vel": vel, "mass": mass},
                  families={"dm": slice(0, 600), "star": slice(600, len(pos))},
                  units_map={"pos": "kpc", "vel": "km s**-1", "mass": "Msol"})
    return sim, reference_fields(pos, vel)


def test_field_codes():
    assert KINEMATIC_FIELDS == ("vr", "vtheta", "vphi", "vrxy", "v2", "vt")
    assert _native.KINEMATIC_FIELDS == KINEMATIC_FIELDS
    assert _native.SRC_KIN == 16


@pytest.mark.parametrize("name", ["vr", "vtheta", "vphi", "vrxy", "v2", "vt"])
def test_fields_bit_for_bit(snap, name):
    sim, ref = snap
    with np.errstate(all="raise"):  # (the host suppresses numpy's warnings itself)
        got = np.asarray(sim[name])
    assert got.dtype == np.float64
    assert np.array_equal(got, ref[name], equal_nan=True)


def test_degenerate_particles_are_nan(snap):
    sim, _ = snap
    n = len(sim) - 2
    for name in ("vr", "vtheta", "vphi", "vrxy", "vt"):
        assert np.isnan(sim[name][n]), name  # the origin: 0/0
    for name in ("vtheta", "vphi", "vrxy"):
        assert np.isnan(sim[name][n + 1]), name  # the z axis: rxy = 0
    assert np.isfinite(sim["vr"][n + 1]) and np.isfinite(sim["v2"][n]) and np.isfinite(sim["v2"][n + 1])


def test_subsnap_views(snap):
    sim, ref = snap
    idx = np.array([5, 17, 400, 999, 1000, 1001])
    sub = sim[idx]
    for name in KINEMATIC_FIELDS:
        assert np.array_equal(np.asarray(sub[name]), ref[name][idx], equal_nan=True)
    star = sim.star
    assert np.array_equal(np.asarray(star["vphi"]), ref["vphi"][600:], equal_nan=True)
    nested = sub[np.array([1, 3])]
    assert np.array_equal(np.asarray(nested["vt"]), ref["vt"][idx[[1, 3]]], equal_nan=True)


def test_units(snap):
    sim, _ = snap
    vel = as_unit("km s**-1")
    for name in ("vr", "vtheta", "vphi", "vrxy", "vt"):
        assert sim[name].units == vel, name
        assert sim.star[name].units == vel, name
    assert sim["v2"].units == vel ** 2
    assert sim["v2"].units == as_unit("km**2 s**-2")
    pos, vel_a, mass = make_arrays(10)
    bare = SimSnap({"pos": pos, "vel": vel_a, "mass": mass})
    assert bare["vr"].units is NoUnit and bare["v2"].units is NoUnit


def test_stored_user_array_wins():
    pos, vel, mass = make_arrays(50)
    sim = SimSnap({"pos": pos, "vel": vel, "mass": mass})
    derived = np.asarray(sim["vr"]).copy()
    mine = np.arange(len(pos), dtype=np.float64)
    sim["vr"] = mine
    assert np.array_equal(np.asarray(sim["vr"]), mine)
    assert np.array_equal(np.asarray(sim[np.array([3, 4])]["vr"]), mine[[3, 4]])
    # the other fields are still derived (vt from the expression, not the stored vr)
    assert np.array_equal(np.asarray(sim["vt"]), reference_fields(pos, vel)["vt"], equal_nan=True)
    assert not np.array_equal(derived, mine)


@pytest.mark.parametrize("name", ["vr", "vtheta", "vphi", "vrxy", "v2", "vt"])
def test_missing_velocities_raise_keyerror(name):
    pos, _, mass = make_arrays(10)
    sim = SimSnap({"pos": pos, "mass": mass})
    with pytest.raises(KeyError) as e:
        sim[name]
    assert e.value.args == (name,)
    with pytest.raises(KeyError):
        sim[np.array([0, 1])][name]


def test_float32_snapshot_stays_float32():
    pos, vel, mass = make_arrays(100)
    p32, v32 = pos.astype(np.float32), vel.astype(np.float32)
    sim = SimSnap({"pos": p32, "vel": v32, "mass": mass})
    ref = reference_fields(p32, v32)  # numpy's float32 arithmetic
    for name in KINEMATIC_FIELDS:
        got = np.asarray(sim[name])
        assert got.dtype == np.float32, name
        assert np.array_equal(got, ref[name], equal_nan=True), name


def test_native_binds_the_kinematic_entry_points():
    names = ["pbx_profile_set_kinematics", "pbx_profile_kinematic_field",
             "pbx_profile_kinematic_moments"]
    bound = _native.exported_symbols()
    for s in names:
        assert s in bound, s
    lib = _native.load()  # (every bound symbol must be exported by the library)
    for s in names:
        assert getattr(lib, s).argtypes is not None, s
    from pynbodyext.profiles._device import SRC_KIN, DeviceBins

    assert [SRC_KIN(f) for f in KINEMATIC_FIELDS] == list(range(16, 22))
    assert DeviceBins.SRC_KIN("vphi") == 18
    with pytest.raises(ValueError):
        SRC_KIN("j")
