"""Property calculators on the device: sums, centres, kappa_rot, ParamContain.

The checker is the numpy restatement of the term table of include/pbx.h
("scalar properties"), written below: per particle the same IEEE operations
in the same order, so only the order of summation differs.  Sums are
compared with np.longdouble sums over the numpy mask within the project's
conditioning bound, 1e-13 x the sum of |term| (as
test_gpu_kinematics.check_sums).
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from oracle import profile_ref as pr
from pynbodyext import _native as nat
from pynbodyext.calculate import ParamView
from pynbodyext.filters import FamilyFilter, Sphere
from pynbodyext.profiles import RadialProfileBuilder
from pynbodyext.profiles._device import DeviceBins
from pynbodyext.properties import (AngMomVec, CenPos, CenVel, KappaRot, KappaRotMean, ParamContain,
                                   ParamSum, PatternSpeed)
from pynbodyext.properties import _device as pdev
from pynbodyext.simcore import SimSnap
from pynbodyext.synthetic import plummer

pytestmark = pytest.mark.gpu

GROUPS = {"mass": (pdev.MASS, [0]), "com": (pdev.COM, [1, 2, 3]), "cov": (pdev.COV, [4, 5, 6]),
          "angmom": (pdev.ANGMOM, [7, 8, 9]), "kappa": (pdev.KAPPA, [10, 11]),
          "kappa_mean": (pdev.KAPPA_MEAN, [12]), "pattern": (pdev.PATTERN, [13, 14, 15, 16, 17])}
ALL = pdev.ALL_GROUPS
CEN, R = (0.3, -0.2, 0.1), 4.0

# The kernel as built (csrc/property.hip): 256 threads x 4 particles per
# sweep and at most 1024 blocks, so one sweep of the full grid covers
# 1024 * 256 * 4 = 1,048,576 particles; one more makes exactly one thread
# start a second sweep.
SWEEP = 1024 * 256 * 4


def reference_terms(pos, vel, mass):
    """The 18 per-particle terms, a list of (n,) arrays; mass None: unit masses."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    vx, vy, vz = vel[:, 0], vel[:, 1], vel[:, 2]
    m = np.ones(len(pos)) if mass is None else mass
    with np.errstate(all="ignore"):
        vc = (x * vy - y * vx) / np.sqrt(x * x + y * y)
        ke = 0.5 * ((vx * vx + vy * vy) + vz * vz)
        return [
            m, x * m, y * m, z * m, vx * m, vy * m, vz * m,
            m * (y * vz - z * vy), m * (z * vx - x * vz), m * (x * vy - y * vx),
            (0.5 * m) * (vc * vc), m * ke, (0.5 * (vc * vc)) / ke,
            (m * x) * x, (m * y) * y, (m * x) * y, m * (x * vy + y * vx), m * (x * vx - y * vy)]


def exact_offset(c, r):
    """x with fl(x - c) == +r or -r exactly (a coordinate at distance r from
    c; on one side the doubles near c + r may all miss it, e.g. c = 0.1, r = 4)."""
    for d in (r, -r):
        x = c + d
        for _ in range(8):
            if x - c == d:
                return x
            x = np.nextafter(x, np.inf if x - c < d else -np.inf)
    raise AssertionError("no representable coordinate")


class Data:
    """A particle set, its numpy mask and the reference sums (built once)."""

    def __init__(self, n, seed, sphere, families, degenerate=(), on_edge=()):
        self.n = n
        if n == 1:
            pos = np.array([[0.3, -0.4, 1.2]])
        else:
            pos, _ = plummer(n, seed=seed)
        rng = np.random.default_rng(seed + 100)
        vel = rng.normal(size=(n, 3))
        mass = rng.uniform(0.5, 1.5, n)
        for i, p in zip(degenerate, ((0.0, 0.0, 0.0), (0.0, 0.0, 1.5))):
            pos[i] = p  # the origin and the z axis (both kept)
        for axis, i in enumerate(on_edge):  # exactly at distance R from the centre
            pos[i] = sphere[0]
            pos[i, axis] = exact_offset(sphere[0][axis], sphere[1])
        self.pos, self.vel, self.mass = pos, vel, mass
        self.sphere, self.families = sphere, families
        keep = np.ones(n, dtype=bool)
        if sphere is not None:
            keep &= pr.sphere_mask(pos, sphere[1], sphere[0])
        if families is not None:
            fam = np.zeros(n, dtype=bool)
            for a, b in families:
                fam[a:b] = True
            keep &= fam
            assert all(fam[i] for i in on_edge)
        self.keep = keep
        assert all(keep[i] for i in degenerate) and not any(keep[i] for i in on_edge)
        self._ref = {}

    def reference(self, unit_mass=False, keep=None):
        """(sums, sum of |term|, NaN flags) in longdouble over the numpy mask."""
        key = (unit_mass, None if keep is None else keep.tobytes())
        if key not in self._ref:
            keep = self.keep if keep is None else keep
            t = reference_terms(self.pos[keep], self.vel[keep], None if unit_mass else self.mass[keep])
            ref, mag = np.zeros(len(t), dtype=np.longdouble), np.zeros(len(t), dtype=np.longdouble)
            nan = np.zeros(len(t), dtype=bool)
            for j, row in enumerate(t):  # (row by row: the longdouble copies stay small)
                nan[j] = np.isnan(row).any()
                tl = np.where(np.isnan(row), 0.0, row).astype(np.longdouble)
                ref[j], mag[j] = tl.sum(), np.abs(tl).sum()
            self._ref[key] = (ref, mag, nan)
        return self._ref[key]

    @functools.cached_property
    def device(self):
        return tuple(nat.DeviceArray.from_host(a) for a in (self.pos, self.vel, self.mass))

    def moments(self, groups, source="host", unit_mass=False, sphere="own", families="own"):
        sphere = self.sphere if sphere == "own" else sphere
        families = self.families if families == "own" else families
        if source == "host":
            return pdev.moments(self.pos, self.vel, None if unit_mass else self.mass, groups=groups,
                                sphere=sphere, families=families)
        dp, dv, dm = self.device
        return pdev.moments(dp.ptr, dv.ptr, None if unit_mass else dm.ptr, groups=groups,
                            sphere=sphere, families=families, on_device=True, n=self.n)


FAMS = [(0, 12000), (14003, 20011)]


@functools.lru_cache(maxsize=None)
def data(name) -> Data:
    if name == "one":  # a single particle
        return Data(1, 1, None, None)
    if name == "tile":  # 4097 kept, one at the origin and one on the z axis
        return Data(4097, 11, ((0.0, 0.0, 0.0), 100.0), None, degenerate=(4095, 4096))
    if name == "fams":  # two family ranges (a gap between them), an off-centre Sphere
        return Data(20011, 12, (CEN, R), FAMS)
    if name == "edge":  # fams plus three particles exactly at distance R: dropped by the strict <
        return Data(20011, 12, (CEN, R), FAMS, on_edge=(100, 5000, 16000))
    if name == "sweep":  # one particle more than one sweep of the full grid
        return Data(SWEEP + 1, 13, None, None)
    if name == "empty":  # nothing kept
        return Data(20011, 12, ((100.0, 100.0, 100.0), 1.0), FAMS)
    raise KeyError(name)


NAMES = ["one", "tile", "fams", "edge", "sweep", "empty"]


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def check_sums(n_kept, got, dat, cols, what, unit_mass=False):
    ref, mag, nan = dat.reference(unit_mass)
    assert n_kept == int(dat.keep.sum()), what
    for j in range(pdev.NSUMS):
        if j not in cols:
            assert got[j] == 0.0 and not np.signbit(got[j]), (what, j)
            continue
        # NaN exactly where a kept particle's term is NaN
        assert bool(np.isnan(got[j])) == bool(nan[j]), (what, j)
        if nan[j]:
            continue
        err = abs(np.longdouble(got[j]) - ref[j])
        print(f"{what} sum {j}: err / Σ|term| = {float(err / max(mag[j], np.longdouble(1e-300))):.2e}")
        assert err <= np.longdouble(1e-13) * mag[j], (what, j)


# ------------------------------------------------------------------ 1. sums
@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("name", NAMES)
def test_sums(gpu, name, source):
    dat = data(name)
    n_kept, sums = dat.moments(ALL, source)
    check_sums(n_kept, sums, dat, range(pdev.NSUMS), f"{name}/{source}/all")
    for g, (bit, cols) in GROUPS.items():
        n_kept, sums = dat.moments(bit, source)
        check_sums(n_kept, sums, dat, cols, f"{name}/{source}/{g}")
    n_kept, sums = dat.moments(ALL, source, unit_mass=True)  # mass = NULL
    check_sums(n_kept, sums, dat, range(pdev.NSUMS), f"{name}/{source}/unit", unit_mass=True)
    if name in ("tile",):  # the degenerate particles are kept: vc is NaN there
        assert np.isnan(sums[10]) and np.isnan(sums[12]) and np.isfinite(sums[11])
    if name == "empty":
        assert n_kept == 0 and np.all(sums == 0.0)


def test_unkept_nan_does_not_leak(gpu):
    """A NaN / inf in a particle outside the sphere or the families never meets a sum."""
    dat = data("fams")
    pos, vel, mass = dat.pos.copy(), dat.vel.copy(), dat.mass.copy()
    out_fam, out_sph = 13000, int(np.nonzero(~dat.keep[:12000])[0][0])
    vel[out_fam] = np.nan
    mass[out_fam] = np.inf
    vel[out_sph] = np.inf
    mass[out_sph] = np.nan
    n_kept, sums = pdev.moments(pos, vel, mass, groups=ALL, sphere=dat.sphere, families=dat.families)
    n0, ref = dat.moments(ALL)
    assert n_kept == n0 and np.array_equal(bits(sums), bits(ref))


# ---------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("name", NAMES)
def test_determinism(gpu, name):
    dat = data(name)
    n1, a = dat.moments(ALL, "host")
    n2, b = dat.moments(ALL, "host")
    n3, c = dat.moments(ALL, "device")
    assert n1 == n2 == n3
    assert np.array_equal(bits(a), bits(b)), "two identical calls"
    assert np.array_equal(bits(a), bits(c)), "host and device inputs"
    for source in ("host", "device"):
        for g, (bit, cols) in GROUPS.items():
            n, s = dat.moments(bit, source)
            assert n == n1 and np.array_equal(bits(s[cols]), bits(a[cols])), (g, source)


# ------------------------------------------------------------ 3. predicate
@pytest.mark.parametrize("name", NAMES)
def test_predicate_agrees_with_select(gpu, name):
    dat = data(name)
    n_kept, _ = dat.moments(pdev.MASS)
    d = DeviceBins.select(dat.pos, dat.mass, sphere=dat.sphere, families=dat.families)
    try:
        assert n_kept == d.n == int(dat.keep.sum())
    finally:
        d.close()
    if name == "edge":  # the three particles at distance R exactly, and their fams twin keeps the same
        assert n_kept == int(data("fams").keep.sum()) - int(data("fams").keep[[100, 5000, 16000]].sum())
        for i, axis in zip((100, 5000, 16000), range(3)):
            d2 = dat.pos[i] - np.asarray(CEN)
            assert (d2[0] * d2[0] + d2[1] * d2[1]) + d2[2] * d2[2] == R * R and abs(d2[axis]) == R


# -------------------------------------------------------- 4. public values
UNITS = {"pos": "kpc", "vel": "km s**-1", "mass": "Msol"}
FAMILY_SLICES = {"dm": slice(0, 12000), "gas": slice(12000, 14003), "star": slice(14003, 20011)}


def snapshot(dat, dtype=np.float64):
    fams = FAMILY_SLICES if dat.n == 20011 else None
    return SimSnap({"pos": dat.pos.astype(dtype), "vel": dat.vel.astype(dtype),
                    "mass": dat.mass.astype(dtype)}, families=fams, units_map=UNITS)


def scope():
    return Sphere(R, cen=CEN) & (FamilyFilter("dm") | FamilyFilter("star"))


def params_of(prop):
    return ParamView({f.name: getattr(prop, f.name) for f in dataclasses.fields(prop)})


PROPS = [ParamSum("mass"), CenPos("com"), CenVel(), AngMomVec(), KappaRot(), KappaRotMean(),
         PatternSpeed()]


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("prop", PROPS, ids=lambda p: type(p).__name__)
def test_public_values(gpu, prop, filtered):
    dat = data("fams")
    sim = snapshot(dat)
    keep = dat.keep if filtered else np.ones(dat.n, dtype=bool)
    calc = prop.filter(scope()) if filtered else prop
    res = calc.run(sim, perf_time=True)
    cls = type(prop).__name__
    assert f"{cls}.device" in res.perf and f"{cls}.calculate" not in res.perf
    n_kept, sums = (dat.moments(ALL) if filtered else dat.moments(ALL, sphere=None, families=None))
    assert n_kept == int(keep.sum())
    want = prop.finish(n_kept, sums, sim)
    assert np.array_equal(bits(res.value), bits(want))
    host = prop.calculate(sim[keep], params_of(prop))
    assert getattr(res.value, "units", None) == getattr(host, "units", None)
    assert np.shape(res.value) == np.shape(host)
    # numpy's sequential axis-0 sum at worst (n 2^-52) plus the device bound
    # through one division (4e-13), times S = Σ|term| / Σm
    ref, mag, _ = dat.reference(keep=keep)
    eps = np.longdouble(int(keep.sum()) * 2.0 ** -52 + 4e-13)
    if cls == "ParamSum":
        assert abs(np.longdouble(float(res.value)) - np.longdouble(float(host))) <= eps * mag[0]
    elif cls in ("CenPos", "CenVel"):
        cols = [1, 2, 3] if cls == "CenPos" else [4, 5, 6]
        for k, j in enumerate(cols):
            tol = eps * mag[j] / ref[0]
            print(f"{cls}[{k}] |device - host| / tol = {float(abs(res.value[k] - host[k]) / tol):.2e}")
            assert abs(np.longdouble(res.value[k]) - np.longdouble(host[k])) <= tol
    elif cls == "KappaRot":
        # the same bound with the ratio's own sums: S = Σ|Krot term| / K
        tol = eps * mag[10] / ref[11]
        print(f"KappaRot |device - host| / tol = {float(abs(res.value - host) / tol):.2e}")
        assert abs(np.longdouble(res.value) - np.longdouble(host)) <= tol


def test_public_values_with_degenerate_particles(gpu):
    """tile keeps a particle at the origin and one on the z axis: kappa is NaN on both routes."""
    dat = data("tile")
    sim = snapshot(dat)
    for prop in (KappaRot(), KappaRotMean()):
        res = prop.run(sim, perf_time=True)
        assert f"{type(prop).__name__}.device" in res.perf and np.isnan(res.value)
        assert np.isnan(prop.calculate(sim[:], params_of(prop)))
    res = CenPos("com").run(sim, perf_time=True)
    n_kept, sums = dat.moments(ALL, sphere=None)
    assert np.array_equal(bits(res.value), bits(sums[1:4] / sums[0]))


def test_empty_selection_is_nan(gpu):
    sim = snapshot(data("fams"))
    nothing = Sphere(1.0, cen=(100.0, 100.0, 100.0)) & FamilyFilter("dm")
    for prop in (CenPos("com"), CenVel(), KappaRot(), KappaRotMean()):
        res = prop.filter(nothing).run(sim, perf_time=True)
        assert f"{type(prop).__name__}.device" in res.perf
        assert np.all(np.isnan(res.value))
    assert ParamSum("mass").filter(nothing)(sim) == 0.0


@pytest.mark.parametrize("prop", PROPS, ids=lambda p: type(p).__name__)
def test_views_and_float32_take_the_host_route(gpu, prop):
    dat = data("fams")
    cls = type(prop).__name__
    view = snapshot(dat)[:]  # a SubSnap input
    res = prop.run(view, perf_time=True)
    assert f"{cls}.device" not in res.perf and f"{cls}.calculate" in res.perf
    assert np.array_equal(bits(res.value), bits(prop.calculate(view, params_of(prop))))
    sim32 = snapshot(dat, np.float32)
    res = prop.run(sim32, perf_time=True)
    assert f"{cls}.device" not in res.perf and f"{cls}.calculate" in res.perf
    assert np.array_equal(np.asarray(res.value), np.asarray(prop.calculate(sim32, params_of(prop))))


# ---------------------------------------------------------- 5. ParamContain
def contain_reference(key, weight, frac):
    """properties/base.py:83-103 with a stable argsort."""
    frac_array = np.asarray([frac] if isinstance(frac, float) else frac, dtype=float)
    order = np.argsort(key, kind="stable")
    key_sorted, weight_sorted = key[order], weight[order]
    cumulative = np.cumsum(weight_sorted)
    denom = float(cumulative[-1] - cumulative[0])
    cumulative = (cumulative - cumulative[0]) / denom
    values = np.interp(frac_array, cumulative, key_sorted)
    return float(values[0]) if isinstance(frac, float) else values


def radius(pos, cal_key):
    return pr.radial_r(pos) if cal_key == "r" else np.sqrt(pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1])


@pytest.mark.parametrize("frac", [0.5, [0.1, 0.5, 0.9]], ids=["scalar", "list"])
@pytest.mark.parametrize("cal_key", ["r", "rxy"])
@pytest.mark.parametrize("name", ["tile", "fams"])
def test_param_contain(gpu, name, cal_key, frac):
    dat = data(name)
    sim = snapshot(dat)
    prop = ParamContain(frac=frac, cal_key=cal_key)
    calc = prop.filter(scope()) if name == "fams" else prop.filter(Sphere(100.0))
    res = calc.run(sim, perf_time=True)
    assert "ParamContain.device" in res.perf and "ParamContain.calculate" not in res.perf
    want = contain_reference(radius(dat.pos, cal_key)[dat.keep], dat.mass[dat.keep], frac)
    assert np.shape(res.value) == np.shape(want)
    assert np.array_equal(bits(res.value), bits(want))
    assert res.value.units == sim["pos"].units and res.value.sim is sim
    if name == "tile":  # unfiltered: the same particles
        assert np.array_equal(bits(prop(sim)), bits(want))


def test_param_contain_ties_are_stable(gpu):
    """Five particles share one radius and differ in mass: index order, as DESIGN states."""
    pos, _ = plummer(200, seed=21)
    mass = np.random.default_rng(22).uniform(0.5, 1.5, 200)
    tied = [150, 3, 77, 40, 199]
    pos[tied] = pos[tied[0]]
    mass[tied] = [1.5, 0.5, 1.25, 0.75, 1.0]
    sim = SimSnap({"pos": pos, "mass": mass}, units_map=UNITS)
    r = pr.radial_r(pos)
    c = np.cumsum(mass[np.argsort(r, kind="stable")])
    lo = int((r < r[tied[0]]).sum())  # the tied five are sorted elements lo .. lo + 4
    assert 1 <= lo < 190
    cdf = (c - c[0]) / (c[-1] - c[0])
    # between the last particle inside and the first of the five (whose mass
    # sets the slope there: the tie order shows), and between the five
    fracs = [0.5 * (cdf[lo + k - 1] + cdf[lo + k]) for k in range(5)] + [0.3, 0.6]
    want = contain_reference(r, mass, fracs)
    other = mass.copy()
    other[[3, 199]] = other[[199, 3]]  # another tie order would give another value
    assert contain_reference(r, other, fracs)[0] != want[0]
    res = ParamContain(frac=fracs).run(sim, perf_time=True)
    assert "ParamContain.device" in res.perf
    assert np.array_equal(bits(res.value), bits(want))


def test_param_contain_small_selections(gpu):
    dat = data("tile")
    sim = snapshot(dat)
    r = np.sort(pr.radial_r(dat.pos))
    assert r[0] == 0.0 < r[1] < r[2] < r[3]
    two = Sphere(0.5 * (r[1] + r[2]))
    got = ParamContain().filter(two).run(sim, perf_time=True)
    assert "ParamContain.device" in got.perf
    keep = pr.sphere_mask(dat.pos, 0.5 * (r[1] + r[2]))
    assert keep.sum() == 2
    assert np.array_equal(bits(got.value), bits(contain_reference(pr.radial_r(dat.pos)[keep], dat.mass[keep], 0.5)))
    with pytest.raises(ValueError, match="Non-positive total 'mass'; cannot compute containment radius."):
        ParamContain().filter(Sphere(0.5 * r[1]))(sim)  # one particle
    with pytest.raises(IndexError):
        ParamContain().filter(Sphere(1.0, cen=(500.0, 0.0, 0.0)))(sim)  # none
    zero = SimSnap({"pos": dat.pos, "mass": np.zeros(dat.n)})
    with pytest.raises(ValueError, match="Non-positive total 'mass'; cannot compute containment radius."):
        ParamContain()(zero)


def test_profile_behind_a_containment_sphere(gpu):
    """Sphere(ParamContain("r", 0.5)) sizes the aperture like the number written in."""
    dat = data("fams")
    sim = snapshot(dat)
    half = ParamContain("r", 0.5)(sim)
    assert float(half) == contain_reference(pr.radial_r(dat.pos), dat.mass, 0.5)
    build = RadialProfileBuilder(ndim=3, weight="mass", bins_type="equaln", nbins=16)
    for calc, number in ((ParamContain("r", 0.5), float(half)), (2 * ParamContain(), 2 * float(half))):
        a = build.filter(Sphere(calc) & FamilyFilter("star"))(sim)
        b = build.filter(Sphere(number) & FamilyFilter("star"))(sim)
        assert len(a.sim) == len(b.sim) > 16
        assert np.array_equal(np.asarray(a.bin_edges), np.asarray(b.bin_edges))
        assert np.array_equal(a.npart_bins, b.npart_bins)
        # per-bin sums accumulate through LDS atomics (order not fixed): each
        # build is within 1e-13 x Σ|term| of the exact sum, the
        # terms are positive masses, so two builds differ by at most 2e-13 x sum
        sa, sb = np.asarray(a["mass"]["sum"]), np.asarray(b["mass"]["sum"])
        assert np.all(np.abs(sa - sb) <= 2e-13 * np.abs(sb))


# ------------------------------------------------------ 6. shrinking sphere
def shrink_reference(pos, mass, min_particles=100, factor=0.7):
    """The loop of simcore.shrink_sphere_center; also the smallest relative
    distance of a membership decision from its sphere."""
    com = (pos.T * mass).sum(axis=1) / mass.sum()
    r = (pos[:, 0].max() - pos[:, 0].min()) / 2
    keep_last = np.ones(len(pos), dtype=bool)
    it, margin = 0, np.inf
    while True:
        dx, dy, dz = pos[:, 0] - com[0], pos[:, 1] - com[1], pos[:, 2] - com[2]
        d2 = (dx * dx + dy * dy) + dz * dz
        keep = d2 < r * r
        margin = min(margin, float(np.min(np.abs(d2 - r * r)) / (r * r)))
        if keep.sum() <= min_particles:
            return com, it, keep_last, margin
        com = (pos[keep].T * mass[keep]).sum(axis=1) / mass[keep].sum()
        keep_last = keep
        r *= factor
        it += 1


def shrink_case(name):
    dat = data(name)
    if name == "fams":  # the families only: 18008 active particles
        act = np.zeros(dat.n, dtype=bool)
        for a, b in FAMS:
            act[a:b] = True
        return dat.pos, dat.mass, FAMS, act
    pos = dat.pos + np.asarray(CEN)
    return pos, dat.mass, None, np.ones(dat.n, dtype=bool)


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("name", ["fams", "tile"])
def test_shrinking_sphere(gpu, name, source):
    pos, mass, fams, act = shrink_case(name)
    ref, it, last, margin = shrink_reference(pos[act], mass[act])
    print(f"{name}: {it} iterations, final count {int(last.sum())}, min |d2 - r2| / r2 = {margin:.2e}")
    assert margin > 1e-9  # no membership decision hangs on rounding
    assert it >= 10 and 100 < last.sum() < len(last)
    x = pos[act][:, 0]
    r0 = float((x.max() - x.min()) / 2)
    if source == "host":
        cen, n_it, n_last = pdev.shrink_center(pos, mass, r0=r0, families=fams)
    else:
        dp, dm = nat.DeviceArray.from_host(pos), nat.DeviceArray.from_host(mass)
        cen, n_it, n_last = pdev.shrink_center(dp.ptr, dm.ptr, r0=r0, families=fams,
                                               on_device=True, n=len(pos))
        dp.free()
        dm.free()
    assert (n_it, n_last) == (it, int(last.sum()))
    p, m = pos[act][last].astype(np.longdouble), mass[act][last].astype(np.longdouble)
    for k in range(3):
        exact = (m * p[:, k]).sum() / m.sum()
        tol = np.longdouble(4e-13) * np.abs(m * p[:, k]).sum() / m.sum()
        print(f"centre[{k}] err / tol = {float(abs(cen[k] - exact) / tol):.2e}")
        assert abs(np.longdouble(cen[k]) - exact) <= tol
    assert np.allclose(cen, ref, rtol=0, atol=1e-12)


def test_shrinking_sphere_public(gpu):
    pos, mass, fams, act = shrink_case("fams")
    sim = SimSnap({"pos": pos, "mass": mass}, families=FAMILY_SLICES, units_map=UNITS)
    x = pos[act][:, 0]
    cen, _, _ = pdev.shrink_center(pos, mass, r0=float((x.max() - x.min()) / 2), families=fams)
    res = CenPos("ssc").filter(FamilyFilter("dm") | FamilyFilter("star")).run(sim, perf_time=True)
    assert "CenPos.device" in res.perf and "CenPos.calculate" not in res.perf
    assert np.array_equal(bits(res.value), bits(cen)) and res.value.units == sim["pos"].units
    ref = shrink_reference(pos[act], mass[act])[0]
    assert np.allclose(res.value, ref, rtol=0, atol=1e-12)
    res = CenPos().run(sim, perf_time=True)  # unfiltered
    assert "CenPos.device" in res.perf
    assert np.allclose(res.value, shrink_reference(pos, mass)[0], rtol=0, atol=1e-12)
    # a Sphere in the scope: the host route
    res = CenPos().filter(Sphere(30.0)).run(sim, perf_time=True)
    assert "CenPos.device" not in res.perf


@pytest.mark.parametrize("n", [100, 101])
def test_shrinking_sphere_few_particles(gpu, n):
    dat = data("tile")
    pos, mass = dat.pos[:n] + np.asarray(CEN), dat.mass[:n]
    ref, it, last, _ = shrink_reference(pos, mass)
    x = pos[:, 0]
    cen, n_it, n_last = pdev.shrink_center(pos, mass, r0=float((x.max() - x.min()) / 2))
    assert (n_it, n_last) == (it, int(last.sum()))
    if n == 100:  # n <= min_particles: the plain centre of mass, no iteration
        assert n_it == 0 and n_last == n
        _, sums = pdev.moments(pos, None, mass, groups=pdev.MASS | pdev.COM)
        assert np.array_equal(bits(cen), bits(sums[1:4] / sums[0]))
    assert np.allclose(cen, ref, rtol=0, atol=1e-13)


# ---------------------------------------------------------------- 7. errors
def raises_value(call):
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) and str(e.value) == nat.last_error()
    return str(e.value)


def test_errors(gpu):
    dat = data("tile")
    pos, vel, mass = dat.pos, dat.vel, dat.mass
    raises_value(lambda: pdev.moments(pos, vel, mass, groups=0))
    raises_value(lambda: pdev.moments(pos, vel, mass, groups=128))
    raises_value(lambda: pdev.moments(pos, vel, mass, groups=ALL | 256))
    for bit in (pdev.COV, pdev.ANGMOM, pdev.KAPPA, pdev.KAPPA_MEAN, pdev.PATTERN):
        assert "vel" in raises_value(lambda bit=bit: pdev.moments(pos, None, mass, groups=bit))
    assert "pos" in raises_value(lambda: pdev.moments(None, vel, mass, groups=pdev.COM))
    assert "pos" in raises_value(lambda: pdev.moments(None, vel, mass, groups=pdev.MASS,
                                                      sphere=((0, 0, 0), 1.0)))
    raises_value(lambda: pdev.moments(None, None, None, groups=pdev.MASS, on_device=True, n=-1))
    many = [(k, k + 1) for k in range(17)]
    raises_value(lambda: pdev.moments(pos, vel, mass, groups=pdev.MASS, families=many))
    # positions are optional when nothing reads them
    n_kept, sums = pdev.moments(None, vel, mass, groups=pdev.MASS | pdev.COV)
    assert n_kept == dat.n and sums[0] > 0
    for r0 in (0.0, -1.0, float("nan")):
        raises_value(lambda r0=r0: pdev.shrink_center(pos, mass, r0=r0))
    for f in (0.0, 1.0, 1.5, -0.5, float("nan")):
        raises_value(lambda f=f: pdev.shrink_center(pos, mass, r0=1.0, shrink_factor=f))
    raises_value(lambda: pdev.shrink_center(pos, mass, r0=1.0, min_particles=0))
    raises_value(lambda: pdev.shrink_center(pos, mass, r0=1.0, families=many))
    d = DeviceBins.select(pos, mass)
    try:
        raises_value(lambda: d.contain([]))
        raises_value(lambda: d.contain(np.full(4097, 0.5)))
        q, out = np.array([0.5]), np.zeros(1)
        den = ctypes.c_double(0.0)
        for w_src in (0, 3, -1):
            raises_value(lambda w_src=w_src: nat.call(
                "pbx_profile_contain", d._h, w_src, None, 1, nat.dptr(q), nat.dptr(out),
                ctypes.byref(den)))
        values, denom = d.contain([0.5], weights=mass)  # a host weight array
        v2, d2 = d.contain([0.5])
        assert values[0] == v2[0] and denom == d2 > 0
    finally:
        d.close()
