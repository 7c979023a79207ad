"""VirialRadius and SpinParam on the device: the enclosed pass
(pbx_property_enclosed), the bisection driver (pbx_property_virial_radius)
and the two properties' device routes.

The checker of the enclosed sums is numpy (tests/_halo_data.py): counts and
extrema exactly, sums against np.longdouble within the project's conditioning
bound, 1e-13 x the sum of |term| (as test_gpu_properties).  The
enclosed pass shares its summation order with the PBX_PROP_MASS sum of
pbx_property_moments_region, so the two are also compared bit for bit.
"""
import functools

import numpy as np
import pytest

import _halo_data as hd
from pynbodyext import _native as nat
from pynbodyext import region as rg
from pynbodyext import simcore
from pynbodyext.filters import Annulus, FamilyFilter, Sphere
from pynbodyext.frame import Frame, apply_half
from pynbodyext.properties import SpinParam, VirialRadius
from pynbodyext.properties import _device as pdev
from pynbodyext.transforms import ShiftPosTo, ShiftVelTo

pytestmark = pytest.mark.gpu

NT = pdev.ENCLOSED_MAX
# The kernel as built (csrc/property.hip, the grid of property_moments): 256
# threads x 4 particles per sweep and at most 1024 blocks, so one sweep of the
# full grid covers 1024 * 256 * 4 = 1,048,576 particles; one more makes
# exactly one thread start a second sweep.
SWEEP = 1024 * 256 * 4
SIZES = [1, 63, 64, 65, 257, 1025, SWEEP + 1]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def ext_equal(got, ref):
    return np.array_equal(got, ref, equal_nan=True)


def check(got, pos, mass, keep, t, what):
    """One enclosed result against numpy: counts and extrema exactly, sums
    within 1e-13 x the sum of |term|."""
    n_kept, msum, count, ext = got
    ref_kept, ref_count, ref_sum, ref_mag, ref_ext = hd.enclosed_reference(pos, mass, keep, t)
    assert n_kept == ref_kept, what
    assert np.array_equal(count, ref_count), what
    if ext is not None:
        assert ext_equal(ext, ref_ext), (what, ext, ref_ext)
    worst = 0.0
    for j in range(len(t)):
        err = abs(np.longdouble(msum[j]) - ref_sum[j])
        assert err <= np.longdouble(1e-13) * ref_mag[j], (what, j, t[j])
        if ref_mag[j] > 0:
            worst = max(worst, float(err / ref_mag[j]))
    print(f"{what}: worst err / sum|term| = {worst:.2e}")


@functools.lru_cache(maxsize=None)
def sample(n):
    pos, _, mass = hd.halo_arrays(n, seed=40 + n % 7)
    return pos, mass


# ------------------------------------------------------------ 1. enclosed
@pytest.mark.parametrize("n", SIZES)
def test_enclosed_sizes(gpu, n):
    pos, mass = sample(n)
    keep = np.ones(n, dtype=bool)
    t = hd.thresholds_for(pos, keep, NT)
    assert len(t) == NT and t[0] == 0.0 and np.isinf(t[2]) and np.isnan(t[3])
    r = hd.radius_of(pos)
    assert (r == t[1]).sum() == 1  # one particle sits exactly on t[1] ...
    host = pdev.enclosed(pos, mass, t)
    check(host, pos, mass, keep, t, f"n={n}")
    n_kept, msum, count, ext = host
    assert count[1] == (r < t[1]).sum() == (r <= t[1]).sum() - 1  # ... and is excluded
    assert count[0] == 0 and msum[0] == 0.0 and count[3] == 0 and msum[3] == 0.0
    assert count[2] == n and n_kept == n
    # arrays resident on the device: the same bits as host staging
    dp, dm = nat.DeviceArray.from_host(pos), nat.DeviceArray.from_host(mass)
    on = dict(on_device=True, n=n)
    dev = pdev.enclosed(dp.ptr, dm.ptr, t, **on)
    assert dev[0] == n_kept and same(dev[1], msum) and np.array_equal(dev[2], count)
    assert ext_equal(dev[3], ext)
    # contract 2: the bits of a sum do not depend on nt, on the other
    # thresholds, on its place in the list or on the extrema
    for j in range(NT):
        one = pdev.enclosed(dp.ptr, dm.ptr, [t[j]], extrema=bool(j % 2), **on)
        assert same(one[1], msum[j:j + 1]) and one[2][0] == count[j] and one[0] == n_kept, j
    pick = [9, 1, 30]
    three = pdev.enclosed(dp.ptr, dm.ptr, t[pick], extrema=False, **on)
    assert three[3] is None and same(three[1], msum[pick]) and np.array_equal(three[2], count[pick])
    # nt = 0: the extrema and the count alone
    none = pdev.enclosed(dp.ptr, dm.ptr, (), **on)
    assert none[0] == n and len(none[1]) == 0 and len(none[2]) == 0 and ext_equal(none[3], ext)
    # the summation order is the PBX_PROP_MASS sum's: the same n particles
    # with the mass zeroed outside the threshold give the same bits
    for j in (range(NT) if n < SWEEP else (1, 2, 9, 17, 30)):
        with np.errstate(invalid="ignore"):
            masked = np.where(r < t[j], mass, 0.0)
        _, sums = pdev.moments(None, None, masked, groups=pdev.MASS)
        assert same(sums[:1], msum[j:j + 1]), (n, j)
    dp.free()
    dm.free()


def test_enclosed_unit_mass(gpu):
    pos, _ = sample(1025)
    keep = np.ones(len(pos), dtype=bool)
    t = hd.thresholds_for(pos, keep, 7)
    got = pdev.enclosed(pos, None, t)
    check(got, pos, None, keep, t, "unit mass")
    assert np.array_equal(got[1], got[2].astype(np.float64))  # (integers: exact)


FAMS = [(0, 12000), (14003, 20011)]
CEN, RADIUS = (0.8, -0.5, 0.3), 60.0
FRAME = Frame(c=(0.3, -0.2, 0.1), R=np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0],
                                               [0.48, 0.64, 0.6]]))
REGION = [rg.sphere_clause((1.0, 2.0, -1.5), 45.0), rg.sphere_clause((0.0, 0.5, 0.0), 4.0, True)]


def test_enclosed_frame_families_sphere_region(gpu):
    """A frame, two family ranges, a Sphere and a two-clause region: numpy on
    the apply_half-transformed arrays; and, bit for bit, the frame-less pass
    on those arrays."""
    n = 20011
    pos, mass = sample(n)
    fpos = apply_half(pos, FRAME.c, FRAME.R)
    fam = np.zeros(n, dtype=bool)
    for a, b in FAMS:
        fam[a:b] = True
    keep = fam & rg.clause_mask(fpos, rg.sphere_clause(CEN, RADIUS)) & rg.region_mask(fpos, REGION)
    assert 0 < keep.sum() < fam.sum() and (fam & ~rg.region_mask(fpos, REGION)).any()
    t = hd.thresholds_for(fpos, keep, NT)
    scope = dict(sphere=(CEN, RADIUS), families=FAMS, region=REGION)
    got = pdev.enclosed(pos, mass, t, frame=FRAME, **scope)
    check(got, fpos, mass, keep, t, "frame+families+sphere+region")
    assert (hd.radius_of(fpos)[keep] == t[1]).sum() == 1
    ref = pdev.enclosed(fpos, mass, t, **scope)
    assert ref[0] == got[0] and same(ref[1], got[1]) and np.array_equal(ref[2], got[2])
    assert ext_equal(ref[3], got[3])
    # each part of the scope alone
    for what, kw, k in (("families", dict(families=FAMS), fam),
                        ("sphere", dict(sphere=(CEN, RADIUS)),
                         rg.clause_mask(pos, rg.sphere_clause(CEN, RADIUS))),
                        ("region", dict(region=REGION), rg.region_mask(pos, REGION)),
                        ("no family", dict(families=[]), np.zeros(n, dtype=bool))):
        check(pdev.enclosed(pos, mass, t[:7], **kw), pos, mass, k, t[:7], what)
    check(pdev.enclosed(pos, mass, t[:7], frame=FRAME), fpos, mass, np.ones(n, dtype=bool), t[:7],
          "frame")


def test_enclosed_nan_coordinate(gpu):
    """A NaN coordinate in a kept particle: NaN extrema of that coordinate and
    of r, the other extrema and every sum as numpy gives them (r is NaN: the
    particle is below no threshold)."""
    n = 4099
    pos, mass = (a.copy() for a in sample(n))
    pos[77, 1] = np.nan
    keep = np.ones(n, dtype=bool)
    t = hd.thresholds_for(pos, keep, 15)
    got = pdev.enclosed(pos, mass, t)
    check(got, pos, mass, keep, t, "nan y")
    ext = got[3]
    assert np.isnan(ext[2]) and np.isnan(ext[3]) and np.isnan(ext[6])
    assert np.isfinite(ext[[0, 1, 4, 5]]).all() and got[0] == n
    # the sums are those of the set without the particle
    clean = np.delete(np.arange(n), 77)
    ref = hd.enclosed_reference(pos[clean], mass[clean], keep[clean], t)
    assert np.array_equal(got[2], ref[1]) and got[2][2] == n - 1
    # an infinite coordinate is an extremum, and r = inf is below no threshold but NaN's
    pos[77] = (np.inf, 0.0, 0.0)
    got = pdev.enclosed(pos, mass, t)
    check(got, pos, mass, keep, t, "inf x")
    assert got[3][1] == np.inf and got[3][6] == np.inf and got[2][2] == n - 1


def test_enclosed_nothing_kept(gpu):
    pos, mass = sample(1025)
    t = [0.0, 10.0, np.inf]
    for kw in (dict(sphere=((1e4, 1e4, 1e4), 1.0)), dict(families=[]),
               dict(region=[rg.cuboid_clause(1e4, 1e4, 1e4, 2e4, 2e4, 2e4)])):
        n_kept, msum, count, ext = pdev.enclosed(pos, mass, t, **kw)
        assert n_kept == 0 and np.all(msum == 0.0) and not np.signbit(msum).any()
        assert np.all(count == 0) and np.isnan(ext).all() and len(ext) == pdev.ENCLOSED_NEXT
    n_kept, msum, count, ext = pdev.enclosed(np.zeros((0, 3)), np.zeros(0), t)
    assert n_kept == 0 and np.all(msum == 0.0) and np.all(count == 0) and np.isnan(ext).all()


def test_enclosed_argument_errors(gpu):
    pos, mass = sample(65)
    with pytest.raises(ValueError, match=r"nt must lie in \[0, 31\]"):
        pdev.enclosed(pos, mass, np.ones(NT + 1))
    with pytest.raises(ValueError, match="at most 8 clauses"):
        pdev.enclosed(pos, mass, [1.0], region=[rg.sphere_clause((0, 0, 0), 1.0)] * 9)
    with pytest.raises(ValueError, match="at most 16 family ranges"):
        pdev.enclosed(pos, mass, [1.0], families=[(0, 1)] * 17)


# --------------------------------------------------------- 2. VirialRadius
def driver(sim, target, **kw):
    return pdev.virial_radius(np.asarray(sim["pos"]), np.asarray(sim["mass"]), target_rho=target,
                              eta=1.0e-3 * target, **kw)


@pytest.mark.parametrize("n,overdensity,seed", hd.VIRIAL_CASES)
def test_virial_radius_cases(gpu, n, overdensity, seed):
    sim, radius, iterations, target = hd.virial_case(n, overdensity, seed)  # (admitted on the CPU)
    prop = VirialRadius(overdensity)
    res = prop.run(sim, perf_time=True)
    assert "VirialRadius.device" in res.perf and "VirialRadius.calculate" not in res.perf
    host = prop(sim, backend="host")
    assert isinstance(res.value, float) and same(res.value, host) and same(host, radius)
    # every L: the same bits and the same iteration count; L = 1 takes one
    # pass per iteration, the chosen L fewer
    by_level = {L: driver(sim, target, levels=L) for L in range(pdev.ENCLOSED_LEVELS + 1)}
    for L, (r, it, passes, n_kept, ok) in by_level.items():
        assert ok and same(r, radius) and it == iterations and n_kept == n, L
        lv = L or pdev.VIRIAL_LEVELS
        assert passes == 1 + -(-iterations // lv), (L, passes)  # (1: the extrema pass)
    assert by_level[0][2] < by_level[1][2]
    print(f"n={n} overdensity={overdensity} seed={seed}: r={radius!r} iterations={iterations} "
          f"passes L=1 {by_level[1][2]}, chosen L {by_level[0][2]}")
    # r_max given: no extrema pass
    x = np.asarray(sim["x"])
    r, it, passes, _, ok = driver(sim, target, r_max=float(x.max() - x.min()))
    assert ok and same(r, radius) and it == iterations and passes == by_level[0][2] - 1


def test_virial_radius_not_converged(gpu):
    sim, overdensity = hd.three_particles()
    with pytest.raises(ValueError, match="Bisection algorithm did not converge"):
        VirialRadius(overdensity)(sim, backend="host")
    with pytest.raises(ValueError, match="Bisection algorithm did not converge"):
        VirialRadius(overdensity)(sim)
    target = simcore.virial_target_density(sim, overdensity)
    for L in (1, 0):
        r, it, passes, n_kept, ok = driver(sim, target, levels=L)
        lv = L or pdev.VIRIAL_LEVELS
        assert not ok and np.isnan(r) and it == 200 and n_kept == 3 and passes == 1 + 200 // lv
    # niter_max is honoured to the iteration: converging needs exactly `iterations`
    sim, radius, iterations, target = hd.virial_case(1000, 2000.0, hd.VIRIAL_SEEDS[0])
    r, it, _, _, ok = driver(sim, target, niter_max=iterations)
    assert ok and same(r, radius) and it == iterations
    r, it, _, _, ok = driver(sim, target, niter_max=iterations - 1)
    assert not ok and np.isnan(r) and it == iterations - 1
    # a negative bracket returns its midpoint at once, as the loop does
    r, it, passes, _, ok = driver(sim, target, r_max=-2.0)
    assert ok and r == -1.0 and it == 0 and passes == 0


def test_virial_radius_argument_errors(gpu):
    sim = hd.halo(1000, hd.VIRIAL_SEEDS[0])
    pos, mass = np.asarray(sim["pos"]), np.asarray(sim["mass"])
    ok = dict(target_rho=1.0, eta=1e-3)
    for bad in (dict(target_rho=np.nan), dict(target_rho=0.0), dict(target_rho=-1.0),
                dict(eta=-1e-3), dict(eta=np.nan), dict(niter_max=0),
                dict(levels=pdev.ENCLOSED_LEVELS + 1), dict(levels=-1)):
        with pytest.raises(ValueError):
            pdev.virial_radius(pos, mass, **{**ok, **bad})


def test_virial_radius_empty_scope(gpu):
    sim = hd.halo(1000, hd.VIRIAL_SEEDS[0])
    for backend in ("host", "mi355x"):
        with pytest.raises(ValueError, match="zero-size array"):
            VirialRadius().filter(Sphere(1e-9))(sim, backend=backend)


SHIFT, BOOST = np.array([30.0, -20.0, 10.0]), np.array([50.0, 10.0, -5.0])


@functools.lru_cache(maxsize=None)
def moved_halo(n=20000, seed=11):
    pos, vel, mass = hd.halo_arrays(n, seed)
    return hd.snapshot(np.ascontiguousarray(pos + SHIFT), np.ascontiguousarray(vel + BOOST), mass)


def test_virial_radius_filter_and_transform(gpu):
    """.filter(FamilyFilter("dm")).transform(frame): the device reads the
    snapshot's own arrays, the family range and the frame in the pass; the
    host builds the framed sub-snapshot.  The same bits."""
    sim = moved_halo()
    frame = ShiftPosTo(SHIFT)
    prop = VirialRadius(500.0).filter(FamilyFilter("dm")).transform(frame)
    # the host route by hand, admitted as the cases are
    dm = sim.family_slice("dm")
    fpos = apply_half(np.asarray(sim["pos"]), SHIFT, None)[dm]
    sub = hd.snapshot(fpos, np.asarray(sim["vel"])[dm], np.asarray(sim["mass"])[dm])
    radius, _, _ = hd.admit(sub, 500.0, "dm in frame")
    res = prop.run(sim, perf_time=True)
    assert "VirialRadius.device" in res.perf
    assert same(res.value, radius) and same(prop(sim, backend="host"), radius)
    # a two-clause region in the scope as well
    scoped = VirialRadius(500.0).filter(FamilyFilter("dm") & Annulus(0.5, 400.0)).transform(frame)
    ring = rg.region_mask(fpos, [rg.sphere_clause((0, 0, 0), 400.0),
                                 rg.sphere_clause((0, 0, 0), 0.5, negate=True)])
    assert 0 < ring.sum() < len(ring)
    sub = hd.snapshot(fpos[ring], np.asarray(sim["vel"])[dm][ring], np.asarray(sim["mass"])[dm][ring])
    radius, _, _ = hd.admit(sub, 500.0, "dm ring in frame")
    res = scoped.run(sim, perf_time=True)
    assert "VirialRadius.device" in res.perf
    assert same(res.value, radius) and same(scoped(sim, backend="host"), radius)


def test_quick_start_lines(gpu):
    """The reference's quick-start lines for the two calculators, unchanged."""
    sim = moved_halo()
    frame = ShiftPosTo("ssc").then(ShiftVelTo("com").filter(Sphere("5 kpc")))
    rvir = VirialRadius(overdensity=200.).transform(frame)(sim)
    lam = SpinParam().filter(Sphere(rvir)).transform(frame)(sim)
    rvir_h = VirialRadius(overdensity=200.).transform(frame)(sim, backend="host")
    lam_h = SpinParam().filter(Sphere(rvir_h)).transform(frame)(sim, backend="host")
    print(f"rvir = {rvir!r} (host {rvir_h!r}), lambda = {lam!r} (host {lam_h!r})")
    # (the centre itself differs in its last bits between the routes)
    assert rvir == pytest.approx(rvir_h, rel=1e-9) and lam == pytest.approx(lam_h, rel=1e-9)
    assert 150.0 < rvir < 200.0 and 0.0 < lam < 1.0
    both = (VirialRadius(200.) * SpinParam()).transform(frame)(sim)
    assert both == pytest.approx(rvir_h * SpinParam().transform(frame)(sim, backend="host"),
                                 rel=1e-9)


# ------------------------------------------------------------ 3. SpinParam
@pytest.mark.parametrize("scope", ["plain", "frame", "filter", "region", "all"])
def test_spin_param(gpu, scope):
    """M, J and R differ from the host's only by the order of summation (R
    not at all): 1e-12 relative."""
    sim = moved_halo() if scope in ("frame", "all") else hd.halo(20000, 11)
    prop = SpinParam()
    if scope in ("filter", "all"):
        prop = prop.filter(Sphere(120.0) & FamilyFilter("dm"))
    if scope == "region":
        prop = prop.filter(Annulus(2.0, 150.0))
    if scope in ("frame", "all"):
        prop = prop.transform(ShiftPosTo(SHIFT).then(ShiftVelTo(BOOST)))
    res = prop.run(sim, perf_time=True)
    assert "SpinParam.device" in res.perf and "SpinParam.calculate" not in res.perf
    host = prop(sim, backend="host")
    print(f"{scope}: device {res.value!r} host {host!r} rel {abs(res.value - host) / host:.2e}")
    assert isinstance(res.value, float) and 0.0 < host < 1.0
    assert abs(res.value - host) <= 1e-12 * host


def test_spin_param_radius_is_exact(gpu):
    sim = hd.halo(20000, 11)
    ext = pdev.enclosed(np.asarray(sim["pos"]), np.asarray(sim["mass"]))[3]
    assert ext[6] == np.asarray(sim["r"]).max()


def test_spin_param_empty_scope(gpu):
    sim = hd.halo(1000, hd.VIRIAL_SEEDS[0])
    for backend in ("host", "mi355x"):
        with pytest.raises(ValueError, match="zero-size array"):
            SpinParam().filter(Sphere(1e-9))(sim, backend=backend)
