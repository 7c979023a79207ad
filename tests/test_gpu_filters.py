"""Filters on the device: the region rides along in the selection and the
property pass (csrc/region.h, pbx_profile_set_region,
pbx_property_moments_region).

The yardstick of a selection is numpy: ``build_mask`` of the filter (the
restatement of include/pbx.h in the same operation order) gives the kept
indices exactly and x to the bit.  With a frame the yardstick is, as in
tests/test_gpu_transforms.py, the same pass on ``Frame.apply`` output.  The
sums of the property pass are checked against extended-precision numpy within
the project's bound, 1e-13 x the sum of |term|.

Particles are a Plummer sphere with the crafted boundary / NaN / infinity
rows of tests/_filters_data.py written over fixed indices; the family ranges
start at a non-zero base.  A kept NaN coordinate (under a negated clause)
gives a NaN x: NaNs are compared by position, not by sign or payload, which
IEEE 754 leaves open for a generated NaN.
"""
import functools

import numpy as np
import pytest

import _filters_data as fd
import _transforms_data as td
from oracle import profile_ref as pr
from pynbodyext import _native as nat
from pynbodyext import region as rg
from pynbodyext.filters import Disc, FamilyFilter, HighPass, Sphere
from pynbodyext.frame import Frame
from pynbodyext.parallel import Communicator
from pynbodyext.profiles import RadialProfileBuilder
from pynbodyext.profiles._device import SRC_NONE, SRC_W, DeviceBins
from pynbodyext.properties import SurfaceDensity, VolumeDensity
from pynbodyext.properties import _device as pdev
from pynbodyext.simcore import SimSnap
from pynbodyext.transforms import ShiftPosTo
from test_gpu_properties import reference_terms

pytestmark = pytest.mark.gpu

C = np.array([0.3, -0.2, 0.1])
VC = np.array([0.05, 0.4, -0.25])
FRAME = Frame(C, VC, td.euler_matrix(0.4, -0.9, 1.7))
WINDOW = {"bin_min": 1e-3, "bin_max": 60.0}  # (keeps a NaN x out of the equaln edges)
SWEEP = 1024 * 256 * 4  # one sweep of the property pass's full grid (csrc/property.hip)
UNITS = {"pos": "kpc", "vel": "km s**-1", "mass": "Msol"}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """Equal to the bit; NaNs at the same places."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(bits(a[ok]), bits(b[ok]))


@functools.lru_cache(maxsize=None)
def particles(n):
    """(pos, vel, mass, family ranges, family mask): crafted row j at index 3 j + 1."""
    from pynbodyext.synthetic import plummer

    if n == 1:
        pos = fd.CRAFTED[13:14].copy()
    else:
        pos, _ = plummer(n, seed=50 + n % 97)
        for j in range(fd.NC):
            if 3 * j + 1 < n:
                pos[3 * j + 1] = fd.CRAFTED[j]
    rng = np.random.default_rng(n)
    vel = rng.normal(size=(n, 3))
    mass = rng.uniform(0.5, 1.5, n)
    fams = None if n < 8 else [(n // 8 + 1, n // 2), (n // 2 + 3, n - n // 10)]
    fam = np.ones(n, dtype=bool)
    if fams:
        fam[:] = False
        for a, b in fams:
            fam[a:b] = True
    for a in (pos, vel, mass, fam):
        a.setflags(write=False)
    return pos, vel, mass, fams, fam


def snap_of(pos):
    n = len(pos)
    return SimSnap({"pos": pos, "mass": np.ones(n)}, units_map=UNITS)


def select(d, pos, mass, spec, fams, frame=None):
    return DeviceBins.select(pos, mass, sphere=spec.get("sphere"), families=fams,
                             region=spec.get("region"), frame=frame, into=d)


# ------------------------------------------------------------ 1. selection
@pytest.mark.parametrize("n", [1, 63, 4097, 70_001])
def test_selection_equals_the_numpy_mask(gpu, n):
    pos, _, mass, fams, fam = particles(n)
    sim = snap_of(pos)
    fpos = FRAME.pos(pos)
    r, fr = pr.radial_r(pos), pr.radial_r(fpos)
    # (a Sphere at the origin: the selection's shortcut, which must AND the region in too)
    cases = {name: f for name, (f, _) in fd.CASES.items()}
    cases["origin"] = Sphere(3.0) & Disc(1.5, 0.5, fd.CEN) & ~Sphere(0.5, fd.CEN)
    d, e = DeviceBins(), DeviceBins()
    try:
        for name in sorted(cases):
            f = cases[name]
            spec = f.device_spec(sim)
            assert spec is not None, name
            for families, fmask in ((None, np.ones(n, dtype=bool)), (fams, fam)):
                if families is None and fams is not None and name.startswith("not_"):
                    continue  # (negations once, with the families)
                keep = np.asarray(f(sim)) & fmask
                select(d, pos, mass, spec, families)
                idx, x, w = d.selection()
                assert np.array_equal(idx, np.flatnonzero(keep)), (n, name)
                assert same_bits(x, r[keep]) and np.array_equal(w, mass[keep]), (n, name)
                # in a frame: the region pass on the rewritten arrays, and numpy on them
                select(d, pos, mass, spec, families, frame=FRAME)
                select(e, fpos, mass, spec, families)
                fi, fx, _ = d.selection()
                ei, ex, _ = e.selection()
                assert np.array_equal(fi, ei) and same_bits(fx, ex), (n, name)
                fkeep = rg.region_mask(fpos, fd.clauses_of(spec)) & fmask
                assert np.array_equal(fi, np.flatnonzero(fkeep)), (n, name)
                assert same_bits(fx, fr[fkeep]), (n, name)
        if n >= 4097:  # the crafted rows did their work
            for name in ("sphere", "disc", "cuboid", "band_r", "annulus", "solar", "and5"):
                got = np.asarray(fd.CASES[name][0](sim))[1:3 * fd.NC:3]
                assert np.array_equal(got, fd.expected_mask(name)), name
        # the region is cleared by a selection without one
        select(d, pos, mass, {}, None)
        assert d.n == n
    finally:
        d.close()
        e.close()


# -------------------------------------------------------- 2. profile paths
@pytest.mark.parametrize("name", ["disc", "annulus", "solar", "cuboid", "not_sphere", "low_r"])
@pytest.mark.parametrize("n", [4097, 70_001])
def test_profile_paths_agree_and_equal_the_oracle(gpu, n, name):
    pos, _, mass, fams, fam = particles(n)
    sim = snap_of(pos)
    f = fd.CASES[name][0]
    spec = f.device_spec(sim)
    keep = np.asarray(f(sim)) & fam
    nbins = 8
    stats = [(SRC_W, SRC_NONE, 1 << 3)]
    ref = pr.radial_profile(pos, mass, keep, "equaln", nbins, **WINDOW)
    dp, dm = nat.DeviceArray.from_host(pos), nat.DeviceArray.from_host(mass)
    d = DeviceBins()
    try:
        results = []
        # the one-launch call on host arrays and on device pointers (lazy)
        for args, kw in (((pos, mass), {}), ((dp.ptr, dm.ptr), {"on_device": True, "n": n})):
            _, edges, counts, mom = DeviceBins.radial_equaln(
                *args, nbins=nbins, sphere=spec.get("sphere"), families=fams,
                region=spec.get("region"), stats=stats, into=d, **WINDOW, **kw)
            results.append((edges, counts, mom[0][:, 3]))
        select(d, pos, mass, spec, fams)
        edges, counts, mom = d.binned_equaln(nbins, WINDOW["bin_min"], WINDOW["bin_max"], stats)
        results.append((edges, counts, mom[0][:, 3]))
        for edges, counts, msum in results:
            assert same_bits(edges, ref["edges"]) and np.array_equal(counts, ref["counts"]), name
            np.testing.assert_allclose(msum, ref["mass_sum"], rtol=1e-12, atol=0)
        assert counts.sum() > nbins
        ps = d.path_stats()
        print(f"n={n} {name}: paths {ps}")
        assert ps["mono"] >= 1, ps  # the one-launch path ran
    finally:
        d.close()
        dp.free()
        dm.free()


def test_lazy_tiled_selection_with_a_region_and_a_frame(gpu):
    """4,194,304 + 5 particles: 1025 selection tiles, the tiled lazy path
    (three calls per handle: the hinted and the speculating variants run, and
    a speculating call rebuilds x from the positions for the reader below)."""
    n = 4_194_304 + 5
    rng = np.random.default_rng(9)
    pos = rng.normal(scale=3.0, size=(n, 3)) + C
    pos[1:3 * fd.NC:3] = fd.CRAFTED
    mass = rng.uniform(0.5, 1.5, n)
    fpos = FRAME.pos(pos)
    region = (Disc(6.0, 2.5, (0.5, -0.25, 0.125)) & ~Sphere(1.0, (0.5, -0.25, 0.125))
              & HighPass("x", -4.0)).device_spec(snap_of(pos[:1]))["region"]
    assert len(region) == 3
    stats = [(SRC_W, SRC_NONE, 1 << 3)]
    out = []
    for arr, frame in ((pos, FRAME), (fpos, None)):
        d = DeviceBins()
        d.set_frame(frame)
        dp, dm = nat.DeviceArray.from_host(arr), nat.DeviceArray.from_host(mass)
        d.set_source_stable(True)
        try:
            calls = []
            for _ in range(3):
                _, e, c, m = DeviceBins.radial_equaln(dp.ptr, dm.ptr, nbins=128,
                                                      sphere=((0.0, 0.0, 0.0), 9.0), region=region,
                                                      on_device=True, n=n, into=d, stats=stats,
                                                      bin_min=0.3, bin_max=8.0)
                calls.append((e, c, m[0]))
            out.append((calls, d.selection(), d.level0_stats(), d.path_stats()))
        finally:
            d.close()
            dp.free()
            dm.free()
    (ca, sa, la, pa), (cb, sb, lb, pb) = out
    assert la["tiled"] == 3 and la == lb, (la, lb)
    assert pa["multi"] == 3 and pa["mono"] == 0 and pa == pb, (pa, pb)
    for (ea, na, ma), (eb, nb_, mb) in zip(ca, cb):
        assert same_bits(ea, eb) and np.array_equal(na, nb_)
        np.testing.assert_allclose(ma, mb, rtol=1e-12, atol=0)  # (float atomics)
    assert np.array_equal(sa[0], sb[0]) and same_bits(sa[1], sb[1]) and same_bits(sa[2], sb[2])
    keep = pr.sphere_mask(fpos, 9.0) & rg.region_mask(fpos, region)
    assert 1000 < keep.sum() < n // 2
    assert np.array_equal(sa[0], np.flatnonzero(keep)) and same_bits(sa[1], pr.radial_r(fpos)[keep])
    ref = pr.radial_profile(fpos, mass, keep, "equaln", 128, 0.3, 8.0)
    assert same_bits(ca[0][0], ref["edges"]) and np.array_equal(ca[0][1], ref["counts"])


# ------------------------------------------------------ 3. the property pass
PROPERTY_CASES = ["annulus", "solar", "cuboid", "disc", "band_x", "and5"]


@pytest.mark.parametrize("n", [1, 63, 1025, 5000, SWEEP + 1000])
def test_property_pass_with_a_region(gpu, n):
    pos, vel, mass, fams, fam = particles(n)
    sim = snap_of(pos)
    fpos, fvel = FRAME.pos(pos), FRAME.vel(vel)
    big = n > 5000  # (the second sweep of the grid: fewer cases)
    # every case: the count alone (a kept NaN row would poison a position sum)
    for name in (["not_disc", "high_r", "and5"] if big else sorted(fd.CASES)):
        spec = fd.CASES[name][0].device_spec(sim)
        keep = np.asarray(fd.CASES[name][0](sim)) & fam
        n_kept, _ = pdev.moments(pos, None, mass, groups=pdev.MASS, sphere=spec.get("sphere"),
                                 families=fams, region=spec.get("region"))
        assert n_kept == int(keep.sum()), (n, name)
    for name in (PROPERTY_CASES[:2] if big else PROPERTY_CASES):
        spec = fd.CASES[name][0].device_spec(sim)
        for frame, p, v in ((None, pos, vel), (FRAME, fpos, fvel)):
            keep = rg.region_mask(p, fd.clauses_of(spec)) & fam
            n_kept, sums = pdev.moments(pos, vel, mass, groups=pdev.ALL_GROUPS,
                                        sphere=spec.get("sphere"), families=fams,
                                        region=spec.get("region"), frame=frame)
            assert n_kept == int(keep.sum()), (n, name, frame is not None)
            for j, row in enumerate(reference_terms(p[keep], v[keep], mass[keep])):
                tl = row.astype(np.longdouble)
                err, mag = abs(np.longdouble(sums[j]) - tl.sum()), np.abs(tl).sum()
                if n == 5000:
                    print(f"{name} frame={frame is not None} sum {j}: "
                          f"err / Σ|term| = {float(err / mag) if mag else 0.0:.2e}")
                assert err <= np.longdouble(1e-13) * mag, (n, name, frame is not None, j)
            if frame is not None:  # and bit for bit the region pass on the rewritten arrays
                ref = pdev.moments(fpos, fvel, mass, groups=pdev.ALL_GROUPS,
                                   sphere=spec.get("sphere"), families=fams,
                                   region=spec.get("region"))
                assert ref[0] == n_kept and same_bits(ref[1], sums), (n, name)
    # the sphere slot, the families and a region together
    spec = (Sphere(3.0) & Disc(2.5, 1.0, fd.CEN) & ~Sphere(0.5, fd.CEN)).device_spec(sim)
    assert set(spec) == {"sphere", "region"} and len(spec["region"]) == 2
    keep = pr.sphere_mask(pos, 3.0) & rg.region_mask(pos, spec["region"]) & fam
    n_kept, sums = pdev.moments(pos, None, mass, groups=pdev.MASS | pdev.COM, sphere=spec["sphere"],
                                families=fams, region=spec["region"])
    assert n_kept == int(keep.sum())
    tl = mass[keep].astype(np.longdouble)
    assert abs(np.longdouble(sums[0]) - tl.sum()) <= np.longdouble(1e-13) * tl.sum()


# ----------------------------------------------------------- 4. error paths
def test_region_errors_and_life_cycle(gpu):
    pos, _, mass, _, _ = particles(4097)
    sim = snap_of(pos)
    region = fd.CASES["annulus"][0].device_spec(sim)["region"]
    nine = [rg.band_clause("x", -float(k + 1), None) for k in range(9)]
    d = DeviceBins()
    try:
        with pytest.raises(ValueError, match="region is set"):
            DeviceBins.select(pos.astype(np.float32), mass, into=d, region=region)
        with pytest.raises(ValueError, match="at most 8 clauses"):
            DeviceBins.select(pos, mass, into=d, region=nine)
        with pytest.raises(ValueError, match="at most 8 clauses"):
            pdev.moments(pos, None, mass, groups=pdev.MASS, region=nine)
        comm = Communicator(1, 0, Communicator.unique_id())
        try:
            with pytest.raises(ValueError, match="region is set"):
                DeviceBins.radial_equaln(pos, mass, nbins=8, comm=comm, into=d, region=region,
                                         **WINDOW)
        finally:
            comm.destroy()
        n, kinds, neg, params = rg.packed(region)
        kinds[0] = 7
        with pytest.raises(ValueError, match="unknown region kind"):
            nat.call("pbx_profile_set_region", d._h, n, kinds, neg, nat.dptr(params))
        n, kinds, neg, params = rg.packed([rg.band_clause("r", 1, 2)])
        params[0, 0] = 9.0
        with pytest.raises(ValueError, match="unknown band field"):
            nat.call("pbx_profile_set_region", d._h, n, kinds, neg, nat.dptr(params))
        # sticky across plain pbx_profile_select calls; cleared by nclauses == 0
        d.set_region(region)
        keep = rg.region_mask(pos, region)
        for _ in range(2):
            kept = nat.c_int64(0)
            args, hold = DeviceBins._select_args(pos, mass, None, None, 3, False, None)
            nat.call("pbx_profile_select", d._h, *args, nat.ctypes.byref(kept))
            assert kept.value == int(keep.sum())
        d.set_region(None)
        DeviceBins.select(pos.astype(np.float32), mass, into=d)  # float32 is accepted again
        assert d.n == 4097
    finally:
        d.close()


# ----------------------------------------------------------- 5. end to end
@pytest.fixture(scope="module")
def disc():
    pos, vel, mass = td.disc_arrays()
    return td.snapshot(pos + np.array([4.0, -2.5, 1.0]), vel, mass)


def test_densities_take_the_device_route_and_equal_the_host_route(gpu, disc):
    frame = ShiftPosTo("com").filter(FamilyFilter("star"))
    for prop in (VolumeDensity("10 kpc", rmin="2 kpc"), SurfaceDensity("10 kpc", "2 kpc")):
        calc = prop.filter(FamilyFilter("star")).transform(frame)
        res = calc.run(disc, perf_time=True)
        cls = type(prop).__name__
        assert f"{cls}.device" in res.perf and f"{cls}.calculate" not in res.perf, sorted(res.perf)
        host = calc.run(disc, backend="host").value
        assert res.value.units == host.units
        # both are one sum of the same kept masses over the same extent: the
        # bound of the sum (1e-13 x the sum of |term|, all terms positive)
        assert abs(float(res.value) - float(host)) <= 1e-13 * abs(float(host)), cls
        assert float(host) > 0
    # another parameter: the host calculate
    res = VolumeDensity("10 kpc", parameter="x").run(disc, perf_time=True)
    assert "VolumeDensity.calculate" in res.perf and "VolumeDensity.device" not in res.perf


def test_profile_behind_disc_and_family(gpu, disc):
    scope = Disc("6 kpc", "0.3 kpc", (4.0, -2.5, 1.0)) & FamilyFilter("star")
    builder = RadialProfileBuilder(weight="mass", bins_type="equaln", nbins=16)
    res = builder.filter(scope).run(disc, perf_time=True)
    assert any(k.endswith("device select") for k in res.perf), sorted(res.perf)
    prof = res.value
    sub = disc[np.asarray(scope(disc))]
    p, m = np.asarray(sub["pos"]), np.asarray(sub["mass"])
    ref = pr.radial_profile(p, m, np.ones(len(p), dtype=bool), "equaln", 16)
    assert same_bits(np.asarray(prof.bin_edges), ref["edges"])
    assert np.array_equal(prof.npart_bins, ref["counts"])
    assert np.array_equal(np.asarray(prof.sim["r"]), pr.radial_r(p))
    assert 1000 < len(p) < td.N_STAR
