"""Frame transforms on the host routes (no GPU).

Every calculator here runs with ``backend="host"`` (or on a sub-snapshot
view), so each property is the reference's numpy ``calculate`` on a
FrameView / materialised snapshot; the checker is the numpy sequence a user
would write by hand (tests/_transforms_data.py, ``example_by_hand``, and the
small restatements below), compared bit for bit.  The device routes and the
profiles are covered by tests/test_gpu_transforms.py.
"""
import numpy as np
import pytest

import _transforms_data as td
from pynbodyext import calculate, transforms
from pynbodyext.calculate import BoundCalculator, RunOptions
from pynbodyext.filters import FamilyFilter, Sphere
from pynbodyext.frame import Frame, FrameView, apply_half, unframe
from pynbodyext.properties import AngMomVec, CenPos, CenVel, KappaRot, ParamContain
from pynbodyext.simcore import SimSnap, SubSnap, calc_faceon_matrix
from pynbodyext.transforms import (AlignAngMomVec, AlignVec, ShiftPosTo, ShiftVelTo, TransformBase,
                                   TransformChain)

HOST = {"backend": "host"}


def small_snap(n=3000, seed=5, dtype=np.float64):
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(n, 3)) * np.array([3.0, 2.0, 1.0]) + np.array([10.0, -5.0, 2.0])
    vel = np.cross([0.3, -0.2, 1.0], pos - np.array([10.0, -5.0, 2.0])) + rng.normal(size=(n, 3))
    vel += np.array([100.0, 0.0, -50.0])
    mass = rng.uniform(0.5, 1.5, n)
    return SimSnap({"pos": pos.astype(dtype), "vel": vel.astype(dtype), "mass": mass.astype(dtype)},
                   families={"dm": slice(0, 1800), "star": slice(1800, n)}, units_map=td.UNITS)


@pytest.fixture(scope="module")
def disc():
    pos, vel, mass = td.disc_arrays()
    mpos, mvel = td.moved(pos, vel)
    return mpos, mvel, mass


def raw(sim, key):
    return np.asarray(sim[key]).copy()


# ------------------------------------------------------------------ surface
def test_exports():
    assert transforms.__all__[:4] == ["AlignVec", "AlignAngMomVec", "ShiftPosTo", "ShiftVelTo"]
    for name in ("TransformBase", "TransformChain", "Frame", "FrameView"):
        assert name in transforms.__all__
    assert not hasattr(transforms, "WrapBox")
    assert isinstance(AlignAngMomVec, AlignVec) and isinstance(AlignAngMomVec.vector, AngMomVec)
    assert hasattr(calculate.CalculatorBase, "transform")
    assert hasattr(calculate.CalculatorBase, "with_transformation")
    assert RunOptions().backend == "mi355x"


def test_constructor_errors():
    with pytest.raises(ValueError, match=r"Invalid mode: nope. Expected one of \['ssc', 'com', 'pot', 'hyb'\]."):
        ShiftPosTo("nope")
    for mode in ("pot", "hyb"):  # as CenPos raises them
        with pytest.raises(NotImplementedError, match=mode):
            ShiftPosTo(mode)
    with pytest.raises(ValueError, match="Invalid mode type: <class 'list'>. Expected str, callable, or array."):
        ShiftPosTo([1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="Invalid mode: ssc. Expected 'com'."):
        ShiftVelTo("ssc")
    with pytest.raises(ValueError, match="Invalid mode type: <class 'tuple'>. Expected str, callable, or array."):
        ShiftVelTo((1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="At least one transform must be provided."):
        TransformChain()
    with pytest.raises(TypeError, match="TransformChain only accepts transform nodes"):
        TransformChain(KappaRot())
    with pytest.raises(ValueError, match="unknown backend 'cuda'"):
        KappaRot()(small_snap(), backend="cuda")
    assert isinstance(ShiftPosTo("ssc").mode, CenPos) and ShiftPosTo("com").description == "com"
    assert isinstance(ShiftVelTo().mode, CenVel) and ShiftPosTo(np.zeros(3)).description == "given"
    assert ShiftPosTo().move_all is True and AlignVec(np.ones(3), move_all=False).move_all is False


def test_chain_building():
    a, b, c = ShiftPosTo("com"), ShiftVelTo("com"), AlignAngMomVec
    chain = a.then(b).then(c)
    assert isinstance(chain, TransformChain) and chain.transforms == (a, b, c)
    assert TransformBase.chain(a, b.then(c)).transforms == (a, b, c)
    f = Sphere(1.0)
    m = b.filter(f)
    assert m is not b and m.measure_filter is f and b.measure_filter is None
    assert b.with_filter(f).measure_filter is f and b.measure_with(f).measure_filter is f
    assert m.measure_with(None).measure_filter is None
    # a bound calculator keeps its transform through .filter(), and chains a second one
    k = KappaRot().transform(a).filter(f)
    assert isinstance(k, BoundCalculator) and k.pre_transform is a and k.pre_filter is f
    k2 = KappaRot().filter(f).transform(a).transform(b, revert=False)
    assert k2.pre_filter is f and k2.pre_transform.transforms == (a, b) and k2.revert is False


# -------------------------------------------------------------------- frame
def test_frame_restatement_and_skipped_steps():
    rng = np.random.default_rng(0)
    a = rng.normal(size=(7, 3))
    a[3] = [np.inf, 1.0, -2.0]
    c = np.array([0.5, -1.0, 2.0])
    rot = td.euler_matrix(0.3, 0.4, 0.5)
    # a step that is not set is skipped: the infinity stays an infinity ...
    got = apply_half(a, c, None)
    assert got[3, 0] == np.inf and np.array_equal(got[3, 1:], a[3, 1:] - c[1:])
    # ... where a rotation by the identity would make NaN of it (0 * inf)
    assert np.isnan(apply_half(a, c, np.eye(3))[3]).sum() == 2
    d = a - c
    want = np.stack([(rot[i, 0] * d[:, 0] + rot[i, 1] * d[:, 1]) + rot[i, 2] * d[:, 2]
                     for i in range(3)], axis=1)
    assert np.array_equal(apply_half(a, c, rot), want, equal_nan=True)
    assert np.array_equal(apply_half(a, None, None), a) and apply_half(a, None, None) is not a
    assert apply_half(a.astype(np.float32), None, None).dtype == np.float64
    fr = Frame(c=c, R=rot)
    assert fr.flags == 1 | 4 and not fr.empty and Frame().empty and Frame().flags == 0
    assert np.array_equal(fr.packed(), np.concatenate([c, np.zeros(3), rot.reshape(9)]))
    # the canonical order, and what leaves it
    assert Frame().with_pos_shift(c).with_vel_shift(c).with_rotation(rot).flags == 7
    assert fr.with_pos_shift(c) is None and fr.with_vel_shift(c) is None
    assert fr.with_rotation(rot) is None and Frame(c=c).with_pos_shift(c) is None
    assert Frame(c=c).with_vel_shift(c).flags == 3


def test_frame_view_passes_other_arrays_through():
    sim = small_snap()
    sim["tag"] = np.arange(len(sim))
    fr = Frame(c=[10.0, -5.0, 2.0], vc=[100.0, 0.0, -50.0], R=td.euler_matrix(1.0, 0.2, -0.4))
    view = FrameView(sim, fr)
    assert unframe(view) == (sim, fr) and unframe(sim) == (sim, None)
    assert np.asarray(view["mass"]).base is np.asarray(sim["mass"]).base or \
        np.shares_memory(view["mass"], sim["mass"])
    assert np.array_equal(view["tag"], np.arange(len(sim)))
    p, v = fr.pos(raw(sim, "pos")), fr.vel(raw(sim, "vel"))
    assert np.array_equal(view["pos"], p) and np.array_equal(view["vel"], v)
    assert np.array_equal(view["x"], p[:, 0]) and np.array_equal(view["vz"], v[:, 2])
    assert np.array_equal(view["r"], np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]))
    plain = SimSnap({"pos": p, "vel": v, "mass": raw(sim, "mass")})
    for key in ("rxy", "vr", "vphi", "vtheta", "vt", "vcxy", "ke"):
        assert np.array_equal(view[key], plain[key], equal_nan=True), key
    assert view["pos"].units == sim["pos"].units and view["vr"].units == sim["vel"].units
    assert view._get_family_slice("star") == sim._get_family_slice("star")
    assert len(view.star) == len(sim.star) and isinstance(view[view["x"] > 0], SubSnap)
    keys_before = sorted(sim.keys())
    for key, value in (("pos", p), ("new", np.zeros(len(sim)))):  # read-only: the snapshot is not written
        with pytest.raises(TypeError, match="a frame view is read-only"):
            view[key] = value
    assert sorted(sim.keys()) == keys_before
    with pytest.raises(TypeError, match="wraps a root snapshot"):
        FrameView(sim[:], fr)
    # materialising: same particles, families, units, float64 pos / vel in the frame
    mat = fr.apply(sim)
    assert type(mat) is SimSnap and np.array_equal(mat["pos"], p) and np.array_equal(mat["vel"], v)
    assert mat._get_family_slice("star") == sim._get_family_slice("star")
    assert mat["pos"].units == sim["pos"].units and np.array_equal(mat["tag"], sim["tag"])
    sub = fr.apply(sim[sim._get_family_slice("star")])
    assert len(sub) == 1200 and len(sub.dm) == 0 and np.array_equal(sub["pos"], p[1800:])


# ------------------------------------------------------------ face-on matrix
def faceon_cases():
    rng = np.random.default_rng(3)
    return [rng.normal(size=3) * 10.0 ** rng.uniform(-3, 6) for _ in range(2000)]


def test_calc_faceon_matrix():
    """Rows orthonormal and R @ (L / |L|) == (0, 0, 1).  Tolerances: over
    these 2000 vectors the construction's float64 matrix, evaluated in
    longdouble, leaves at most 2.3e-16 in R @ (L / |L|) - z and 6.5e-16 in
    R @ R.T - 1 (measured on the CPU); the bounds are those with a margin of 4."""
    ld = np.longdouble
    worst_z = worst_o = ld(0)
    for vec in faceon_cases():
        rot = calc_faceon_matrix(vec, up=AlignVec._safe_up(vec))
        assert rot.shape == (3, 3) and rot.dtype == np.float64
        rl, vl = rot.astype(ld), vec.astype(ld)
        unit = vl / np.sqrt((vl * vl).sum())
        worst_z = max(worst_z, np.abs(rl @ unit - np.array([0, 0, 1], dtype=ld)).max())
        worst_o = max(worst_o, np.abs(rl @ rl.T - np.eye(3, dtype=ld)).max())
    print(f"face-on: |R u - z| <= {float(worst_z):.2e}, |R R^T - 1| <= {float(worst_o):.2e}")
    assert worst_z <= 4 * 2.3e-16 and worst_o <= 4 * 6.5e-16
    # pynbody's construction: rows p1 = up x vec, p2 = vec x p1, vec (normalised)
    rot = calc_faceon_matrix([0.0, 0.0, 2.0], up=[0.0, 1.0, 0.0])
    assert np.array_equal(rot, np.eye(3))
    rot = calc_faceon_matrix([3.0, 0.0, 0.0], up=[0.0, 1.0, 0.0])
    assert np.array_equal(rot, [[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])


def test_safe_up():
    up = AlignVec._safe_up
    assert np.array_equal(up([0.0, 0.0, 5.0]), [0.0, 1.0, 0.0])
    # up parallel to the vector: the axis least aligned with it
    assert np.array_equal(up([0.0, 3.0, 0.0]), [1.0, 0.0, 0.0])
    assert np.array_equal(up([0.1, -7.0, 0.2]), [0.0, 1.0, 0.0])  # (not within 1e-6 of parallel)
    assert np.array_equal(up([1e-9, -7.0, 2e-9]), [1.0, 0.0, 0.0])
    assert np.array_equal(up([1.0, 0.0, 0.0], up=[2.0, 0.0, 0.0]), [0.0, 1.0, 0.0])
    assert np.allclose(up([1.0, 0.0, 0.0], up=[0.0, 0.0, 4.0]), [0.0, 0.0, 1.0])
    assert np.array_equal(up([1.0, 0.0, 0.0], up=[0.0, 0.0, 0.0]), [0.0, 1.0, 0.0])  # a zero up: the default
    for bad in ([0.0, 0.0, 0.0], [np.nan, 1.0, 0.0]):
        with pytest.raises(ValueError, match="Angular momentum vector is zero or NaN"):
            up(bad)
    with pytest.raises(ValueError, match="Angular momentum vector is zero or NaN"):
        KappaRot().transform(AlignVec(np.zeros(3)))(small_snap(), **HOST)


# ------------------------------------------------------------------ chains
def test_measure_filter_is_evaluated_in_the_frame_so_far():
    """ShiftVelTo("com").filter(Sphere(r)) after ShiftPosTo(c) measures inside
    the sphere about c — not about the stored origin — and shifts everyone."""
    sim = small_snap()
    pos, vel, mass = raw(sim, "pos"), raw(sim, "vel"), raw(sim, "mass")
    c = np.array([10.0, -5.0, 2.0])
    t = ShiftPosTo(c).then(ShiftVelTo("com").filter(Sphere(2.0)))
    framed = t(sim, **HOST)
    assert isinstance(framed, FrameView) and framed._frame.R is None
    d = pos - c
    inside = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < 4.0
    assert 100 < inside.sum() < len(sim)
    about_origin = ((pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]) + pos[:, 2] * pos[:, 2]) < 4.0
    assert about_origin.sum() == 0  # (the stored origin's sphere is empty: it was not used)
    vc = (vel[inside].T * mass[inside]).sum(axis=-1) / mass[inside].sum()
    assert np.array_equal(framed._frame.c, c) and np.array_equal(framed._frame.vc, vc)
    assert len(framed) == len(sim)  # the measure filter did not narrow the snapshot
    assert np.array_equal(framed["vel"], vel - vc) and np.array_equal(framed["pos"], d)
    # a callable parameter sees the filtered view of the frame so far
    seen = {}

    def mean_velocity(s):
        seen["n"], seen["x"] = len(s), np.asarray(s["x"]).copy()
        return s.mean_by_mass("vel")

    g = ShiftPosTo(c).then(ShiftVelTo(mean_velocity).filter(Sphere(2.0)))(sim, **HOST)
    assert seen["n"] == inside.sum() and np.array_equal(seen["x"], d[inside, 0])
    assert np.array_equal(g._frame.vc, vc)


def test_larger_example_equals_the_hand_written_sequence(disc):
    mpos, mvel, mass = disc
    sim = td.snapshot(mpos, mvel, mass)
    before = {k: raw(sim, k).tobytes() for k in ("pos", "vel", "mass")}
    kappa, (c, vc, rot), p2, v2 = td.example_by_hand(mpos, mvel, mass)
    res = td.example().run(sim, perf_time=True, **HOST)
    assert res.value == float(kappa)
    assert "KappaRot.calculate" in res.perf and not any(k.endswith(".device") for k in res.perf)
    framed = td.example_transform()(sim, **HOST)
    fr = framed._frame
    assert np.array_equal(fr.c, c) and np.array_equal(fr.vc, vc) and np.array_equal(fr.R, rot)
    assert np.array_equal(framed["pos"], p2) and np.array_equal(framed["vel"], v2)
    # revert=True (the default): the snapshot is untouched, byte for byte
    assert all(raw(sim, k).tobytes() == b for k, b in before.items())
    # a sub-snapshot view and float32 inputs materialise first; the same numbers
    # (float32 widened exactly: the frame is float64 arithmetic)
    assert td.example()(sim[:], **HOST) == float(kappa)
    s32 = td.snapshot(mpos.astype(np.float32), mvel.astype(np.float32), mass)
    k32 = td.example_by_hand(mpos.astype(np.float32).astype(np.float64),
                             mvel.astype(np.float32).astype(np.float64), mass)[0]
    assert td.example()(s32, **HOST) == float(k32)
    # it is the disc's own frame: the known rotation's third row, up to the disc's noise
    assert abs(np.dot(rot[2], td.euler_matrix(*td.ANGLES)[:, 2])) > 0.999


def test_non_canonical_chains_materialise():
    sim = small_snap()
    pos, vel, mass = raw(sim, "pos"), raw(sim, "vel"), raw(sim, "mass")
    c1 = np.array([1.0, 2.0, 3.0])
    t = (ShiftPosTo(c1).then(ShiftPosTo("com"))           # a second shift of pos
         .then(AlignAngMomVec).then(ShiftVelTo("com"))    # a shift after a rotation
         .then(AlignVec(AngMomVec(), up=[1.0, 0.0, 0.0])))  # a second rotation
    framed = t(sim, **HOST)
    # sequential numpy application
    p = td._shift(pos, c1)
    p = td._shift(p, (p.T * mass).sum(axis=-1) / mass.sum())
    ang = (mass.reshape((len(mass), 1)) * np.cross(p, vel)).sum(axis=0)
    r1 = calc_faceon_matrix(ang, up=AlignVec._safe_up(ang))
    p, v = td._rotate(p, r1), td._rotate(vel, r1)
    v = td._shift(v, (v.T * mass).sum(axis=-1) / mass.sum())
    ang = (mass.reshape((len(mass), 1)) * np.cross(p, v)).sum(axis=0)
    r2 = calc_faceon_matrix(ang, up=[1.0, 0.0, 0.0])
    p, v = td._rotate(p, r2), td._rotate(v, r2)
    assert np.array_equal(framed["pos"], p) and np.array_equal(framed["vel"], v)
    # the chain went on from materialised snapshots (the second position shift,
    # then the velocity shift after the first rotation); what is left is that
    # velocity shift and the last rotation, a canonical frame again
    assert isinstance(framed, FrameView) and framed._frame.flags == 2 | 4
    assert framed._frame_base is not sim and np.array_equal(framed._frame.R, r2)
    assert framed._frame_base._get_family_slice("star") == sim._get_family_slice("star")
    x, y, vx, vy, vz = p[:, 0], p[:, 1], v[:, 0], v[:, 1], v[:, 2]
    vcxy = (x * vy - y * vx) / np.sqrt(x * x + y * y)
    want = np.sum(0.5 * mass * (vcxy ** 2)) / np.sum(mass * (0.5 * ((vx * vx + vy * vy) + vz * vz)))
    assert KappaRot().transform(t)(sim, **HOST) == float(want)
    assert np.array_equal(raw(sim, "pos"), pos) and np.array_equal(raw(sim, "vel"), vel)


def test_revert_false_rewrites_the_snapshot(disc):
    mpos, mvel, mass = disc
    kappa, _, p2, v2 = td.example_by_hand(mpos, mvel, mass)
    sim = td.snapshot(mpos.copy(), mvel.copy(), mass.copy())
    pos_buffer = sim._arrays["pos"]
    _ = sim["r"]  # (a derived field cached before the rewrite)
    got = KappaRot().filter(td.example_scope()).transform(td.example_transform(), revert=False)(
        sim, **HOST)
    assert got == float(kappa)
    assert sim._arrays["pos"] is pos_buffer  # in place
    assert np.array_equal(raw(sim, "pos"), p2) and np.array_equal(raw(sim, "vel"), v2)
    assert np.array_equal(raw(sim, "mass"), mass)
    assert np.array_equal(sim["r"], np.sqrt((p2[:, 0] * p2[:, 0] + p2[:, 1] * p2[:, 1])
                                            + p2[:, 2] * p2[:, 2]))
    # in the disc's frame now: the plain calculator gives the same number
    assert KappaRot().filter(td.example_scope())(sim, **HOST) == float(kappa)
    # a view: its particles' rows of the root are rewritten, the others stay
    sim2 = td.snapshot(mpos.copy(), mvel.copy(), mass.copy())
    stars = sim2[td.STAR]
    c = np.array([1.0, 2.0, 3.0])
    ParamContain("r").transform(ShiftPosTo(c), revert=False)(stars, **HOST)
    assert np.array_equal(raw(sim2, "pos")[td.STAR], mpos[td.STAR] - c)
    assert np.array_equal(raw(sim2, "pos")[:td.N_DM], mpos[:td.N_DM])
    assert np.array_equal(raw(stars, "pos"), mpos[td.STAR] - c)


def test_nested_runs_inherit_the_backend():
    """A Sphere radius given as a calculator is evaluated by a run of its own;
    it inherits backend="host" (no device is touched in this file)."""
    sim = small_snap()
    half = ParamContain("r")
    assert half.frac == 0.5 and half.cal_key == "r"
    got = ParamContain("r").filter(Sphere(2 * half, cen=CenPos("com")))(sim, **HOST)
    pos, mass = raw(sim, "pos"), raw(sim, "mass")
    cen = (pos.T * mass).sum(axis=-1) / mass.sum()
    r = np.sqrt((pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]) + pos[:, 2] * pos[:, 2])
    radius = 2 * td._half_mass_radius(pos, mass)
    d = pos - cen
    keep = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < radius * radius
    assert got == td._half_mass_radius(pos[keep], mass[keep]) and 0 < keep.sum()
    assert r[keep].size == keep.sum()


def test_calculator_layer_additions():
    """What the transforms needed of the existing classes: arithmetic on a
    scoped property, ParamContain by field alone, options and phases of a
    nested run, the backend check."""
    sim = small_snap()
    view = sim[:]
    pos, mass = raw(sim, "pos"), raw(sim, "mass")
    half = td._half_mass_radius(pos, mass)
    scoped = ParamContain("r").filter(FamilyFilter("star"))
    assert isinstance(scoped, BoundCalculator)
    star_half = td._half_mass_radius(pos[1800:], mass[1800:])
    assert scoped(view) == star_half
    assert (0.5 * scoped)(view) == 0.5 * star_half and (scoped / 4)(view) == star_half / 4
    assert (scoped + ParamContain())(view) == star_half + half and (-scoped)(view) == -star_half
    assert (2 - scoped)(view) == 2 - star_half and (scoped * scoped)(view) == star_half * star_half
    p = ParamContain("rxy")
    assert (p.frac, p.cal_key) == (0.5, "rxy") and ParamContain()(view) == half
    # a nested run (the Sphere's radius) inherits perf_time and reports into the outer run
    res = KappaRot().filter(Sphere(2 * ParamContain()))
    out = res.run(sim, perf_time=True, **HOST)
    assert "ParamContain.calculate" in out.perf and "KappaRot.calculate" in out.perf
    assert res.run(sim, **HOST).perf == {}
    # options given to a run are not inherited by a later, separate run
    assert "KappaRot.calculate" not in KappaRot().run(view).perf
    for bad in ("cuda", ""):
        with pytest.raises(ValueError, match="unknown backend"):
            KappaRot().run(view, backend=bad)
