"""Kinematic fields on the device: vr, vtheta, vphi, vrxy, v2, vt and beta.

The checker is the numpy restatement of the definitions (float64, no FMA,
these expressions in this order), written below.  Per-particle values must
equal numpy's bit for bit: the same IEEE operations, correctly rounded `/`
and sqrt.  Per-bin sums are compared with extended-precision numpy sums over
the oracle's bin membership within the project's conditioning bound,
1e-13 x the bin's sum of |term|, per bin and column.
"""
import functools

import numpy as np
import pytest

from oracle import profile_ref as pr
from pynbodyext import _native as nat
from pynbodyext.filters import FamilyFilter, Sphere
from pynbodyext.profiles import RadialProfileBuilder
from pynbodyext.profiles._device import ALL_COLS, NMOM, SRC_KIN, SRC_NONE, SRC_W, DeviceBins
from pynbodyext.profiles.proarray import ProfileArray
from pynbodyext.simcore import KINEMATIC_FIELDS, SimSnap, is_pending
from pynbodyext.synthetic import plummer

pytestmark = pytest.mark.gpu

W, FW, F2W, F, F2, AW, A = range(7)
WEIGHTED_COLS = (W, FW, F2W, AW)


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


class Data:
    """A particle set, its selection and the reference fields (built once)."""

    def __init__(self, n, seed, sphere, families, degenerate):
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
        self.idx = np.nonzero(keep)[0]
        assert all(i in self.idx for i in degenerate)
        self.fields = reference_fields(pos, vel)
        self.r = pr.radial_r(pos)


@functools.lru_cache(maxsize=None)
def data(name) -> Data:
    if name == "one":  # a single particle
        return Data(1, 1, None, None, ())
    if name == "tile":  # 4097 kept: one more than a 4096-slot selection tile
        return Data(4097, 11, ((0.0, 0.0, 0.0), 100.0), None, (4095, 4096))
    if name == "fams":  # two families (a gap between them), an off-centre Sphere
        return Data(20011, 12, ((0.3, -0.2, 0.1), 4.0), [(0, 12000), (14003, 20011)], (7, 15000))
    raise KeyError(name)


class Handle:
    """A DeviceBins over a Data set, by handle kind, with kinematics registered."""

    def __init__(self, dat: Data, kind: str, nbins: int | None = None):
        self.dat, self.kind = dat, kind
        self.keep = []  # device arrays borrowed by the handle
        n = dat.n
        if kind == "eager":
            self.dev = DeviceBins.select(dat.pos, dat.mass, sphere=dat.sphere, families=dat.families)
        elif kind == "lazy":
            self.dev, self.edges, self.counts, _ = DeviceBins.radial_equaln(
                dat.pos, dat.mass, nbins=nbins or 8, sphere=dat.sphere, families=dat.families)
        elif kind == "ondev":
            dp, dm, dv = (nat.DeviceArray.from_host(a) for a in (dat.pos, dat.mass, dat.vel))
            self.keep = [dp, dm, dv]
            self.dev, self.edges, self.counts, _ = DeviceBins.radial_equaln(
                dp.ptr, dm.ptr, nbins=nbins or 8, sphere=dat.sphere, families=dat.families,
                on_device=True, n=n)
        elif kind == "from_x":
            self.dev = DeviceBins.from_x(dat.r)
        else:
            raise KeyError(kind)
        self.idx = np.arange(n) if kind == "from_x" else dat.idx
        assert self.dev.n == len(self.idx)
        if kind == "ondev":
            self.dev.set_kinematics(self.keep[0].ptr, self.keep[2].ptr, on_device=True, n=n)
        else:
            self.dev.set_kinematics(dat.pos, dat.vel)
        self.w = dat.mass[self.idx]
        # the weights on the device: the selection's, or a host array
        self.wsrc = self.w if kind == "from_x" else SRC_W

    def bin(self, nbins):
        """equaln bins; returns the oracle's bin id of every kept particle."""
        d = self.dev
        if self.kind in ("lazy", "ondev"):  # (the one-call path's own bins)
            assert d.nbins == nbins
            edges, counts = self.edges, self.counts
        else:
            edges = d.edges_equaln(nbins)
            counts = d.assign(edges)
        x = self.dat.r[self.idx]
        assert np.array_equal(edges, pr.edges_equaln(x, nbins))
        b = pr.bin_ids(x, edges)
        assert np.array_equal(counts, np.bincount(b, minlength=nbins + 1)[:nbins])
        return b

    def close(self):
        self.dev.close()
        for a in self.keep:
            a.free()


def reference_sums(f, w, b, nb):
    """(sums, magnitudes) (nb, 7) of one field: Σ term and Σ |term| per bin in
    extended precision (the reference's own error is then negligible against
    the bound); a NaN term makes its bin's sum NaN.  w None: unweighted (the
    weighted columns are 0)."""
    ww = np.ones_like(f) if w is None else w
    with np.errstate(all="ignore"):
        terms = [ww, f * ww, (f * f) * ww, f, f * f, np.abs(f) * ww, np.abs(f)]
    order = np.argsort(b, kind="stable")
    bs = b[order]
    starts = np.searchsorted(bs, np.arange(nb))
    stops = np.searchsorted(bs, np.arange(nb), side="right")
    sums, mags = np.zeros((nb, NMOM)), np.zeros((nb, NMOM))
    for j, t in enumerate(terms):
        if w is None and j in WEIGHTED_COLS:
            continue
        t = t[order].astype(np.longdouble)
        for k in range(nb):
            seg = t[starts[k]:stops[k]]
            sums[k, j] = float(seg.sum())
            mags[k, j] = float(np.abs(seg).sum())
    return sums, mags


def check_sums(got, f, w, b, nb, what):
    ref, mag = reference_sums(f, w, b, nb)
    nan_bins = np.zeros(nb, dtype=bool)
    nan_bins[b[np.isnan(f) & (b < nb)]] = True
    for j in range(NMOM):
        if w is None and j in WEIGHTED_COLS:
            assert np.all(got[:, j] == 0.0), (what, j)
            continue
        # NaN in exactly the bins that hold a NaN particle (Σw never)
        want_nan = nan_bins if j != W else np.zeros(nb, dtype=bool)
        assert np.array_equal(np.isnan(got[:, j]), want_nan), (what, j)
        ok = ~want_nan
        err = np.abs(got[ok, j] - ref[ok, j])
        print(f"{what} col {j}: max err / Σ|term| = "
              f"{np.max(err / np.maximum(mag[ok, j], 1e-300), initial=0.0):.2e}")
        assert np.all(err <= 1e-13 * mag[ok, j]), (what, j)
    return mag


# --------------------------------------------------------------- per particle
@pytest.mark.parametrize("name,kind", [("one", "eager"), ("one", "from_x"), ("tile", "eager"),
                                       ("tile", "lazy"), ("tile", "ondev"), ("tile", "from_x"),
                                       ("fams", "eager"), ("fams", "lazy"), ("fams", "ondev"),
                                       ("fams", "from_x")])
def test_field_values_bit_for_bit(gpu, name, kind):
    dat = data(name)
    h = Handle(dat, kind)
    try:
        for f in KINEMATIC_FIELDS:
            got = h.dev.kinematic_field(f)
            assert np.array_equal(got, dat.fields[f][h.idx], equal_nan=True), f
        if name != "one":  # the degenerate particles are kept and NaN
            assert np.isnan(h.dev.kinematic_field("vphi")).sum() >= 2
    finally:
        h.close()


# ------------------------------------------------------------------ per bin
MOMENT_CASES = [("one", "eager", 1, True), ("one", "from_x", 1, False),
                ("tile", "eager", 1, True), ("tile", "lazy", 8, False), ("tile", "from_x", 8, True),
                ("tile", "ondev", 128, True),
                ("fams", "eager", 8, False), ("fams", "eager", 128, True),
                ("fams", "lazy", 1, True), ("fams", "lazy", 128, False), ("fams", "ondev", 8, True),
                ("fams", "from_x", 128, True),
                # 6 fields x 6 columns + Σw = 37 slots x 200 bins > 800 x 7: the fallback
                ("fams", "eager", 200, True), ("fams", "lazy", 200, False)]


@pytest.mark.parametrize("name,kind,nbins,weighted", MOMENT_CASES)
def test_fused_and_generic_sums(gpu, name, kind, nbins, weighted):
    dat = data(name)
    h = Handle(dat, kind, nbins)
    try:
        if name == "one":  # (one value: explicit edges)
            counts = h.dev.assign(np.array([0.0, 10.0]))
            assert counts.tolist() == [1]
            b = np.zeros(1, dtype=np.int64)
        else:
            b = h.bin(nbins)
        w = h.w if weighted else None
        wsrc = h.wsrc if weighted else SRC_NONE
        fused = h.dev.kinematic_moments(KINEMATIC_FIELDS, wsrc, ALL_COLS)
        assert fused.shape == (6, nbins, NMOM)
        for k, f in enumerate(KINEMATIC_FIELDS):
            vals = dat.fields[f][h.idx]
            mag = check_sums(fused[k], vals, w, b, nbins, f"fused {f}")
            generic = h.dev.moments(SRC_KIN(f), wsrc, ALL_COLS)
            check_sums(generic, vals, w, b, nbins, f"generic {f}")
            # the two paths agree within the same bound
            ok = ~np.isnan(generic)
            assert np.array_equal(np.isnan(fused[k]), ~ok), f
            assert np.all(np.abs(fused[k] - generic)[ok] <= 1e-13 * mag[ok]), f
    finally:
        h.close()


@pytest.mark.parametrize("kind,weighted", [("eager", True), ("lazy", False)])
def test_unrequested_columns_are_zero(gpu, kind, weighted):
    dat = data("fams")
    h = Handle(dat, kind, 16)
    try:
        b = h.bin(16)
        w = h.w if weighted else None
        wsrc = h.wsrc if weighted else SRC_NONE
        # the beta request (three fields' Σf²w and the shared Σw), then mixed masks
        for fields, cols in [(("vr", "vtheta", "vphi"), [1 << F2W | 1 << W] * 3),
                             (("v2", "vt", "vr", "vr"), [1 << F, 0, 1 << A | 1 << FW, 1 << W])]:
            got = h.dev.kinematic_moments(fields, wsrc, cols)
            for k, (f, c) in enumerate(zip(fields, cols)):
                full, mag = reference_sums(dat.fields[f][h.idx], w, b, 16)
                for j in range(NMOM):
                    asked = bool(c & (1 << j)) and (weighted or j not in WEIGHTED_COLS)
                    if not asked:
                        assert np.all(got[k, :, j] == 0.0), (f, j)
                        continue
                    ok = ~np.isnan(full[:, j])
                    assert np.array_equal(np.isnan(got[k, :, j]), ~ok), (f, j)
                    assert np.all(np.abs(got[k, :, j] - full[:, j])[ok] <= 1e-13 * mag[ok, j]), (f, j)
    finally:
        h.close()


@pytest.mark.parametrize("kind", ["eager", "lazy", "from_x"])
def test_percentiles_of_a_kinematic_source(gpu, kind):
    dat = data("fams")
    h = Handle(dat, kind, 16)
    try:
        h.bin(16)
        q = [0.16, 0.5, 0.84]
        for f, wsrc, absval in (("vr", h.wsrc, False), ("vt", SRC_NONE, False), ("vphi", h.wsrc, True)):
            host = dat.fields[f][h.idx]
            a = h.dev.percentiles(q, SRC_KIN(f), wsrc, absval=absval)
            c = h.dev.percentiles(q, host, wsrc, absval=absval)
            assert np.array_equal(a, c, equal_nan=True), f
            assert np.isfinite(a).any()
    finally:
        h.close()


# ------------------------------------------------------------------- errors
def test_errors(gpu):
    dat = data("fams")
    d = DeviceBins.select(dat.pos, dat.mass, sphere=dat.sphere, families=dat.families)
    try:
        d.assign(d.edges_equaln(8))
        for call in (lambda: d.moments(SRC_KIN("vr"), SRC_W), lambda: d.kinematic_field("vr"),
                     lambda: d.percentiles([0.5], SRC_KIN("vr")),
                     lambda: d.kinematic_moments(["vr"], SRC_W)):
            with pytest.raises(ValueError, match="no kinematics registered"):
                call()
        # n must be the length of the arrays the selection was made from
        with pytest.raises(ValueError, match="selection was made from 20011"):
            d.set_kinematics(dat.pos[:-1], dat.vel[:-1])
        assert not d.has_kinematics
        d.set_kinematics(dat.pos, dat.vel)
        assert np.isfinite(d.moments(SRC_KIN("vr"), SRC_W)[:, FW]).any()
        with pytest.raises(ValueError, match="1 to 6 kinematic fields"):
            d.kinematic_moments(["vr"] * 7, SRC_W)
        # a NULL pair clears the registration; so does a new selection
        d.set_kinematics(None, None)
        with pytest.raises(ValueError, match="no kinematics registered"):
            d.kinematic_field("vr")
        d.set_kinematics(dat.pos, dat.vel)
        DeviceBins.select(dat.pos, dat.mass, sphere=dat.sphere, into=d)
        with pytest.raises(ValueError, match="no kinematics registered"):
            d.kinematic_field("vr")
        x = DeviceBins.from_x(dat.r[:100])
        with pytest.raises(ValueError, match="selection was made from 100"):
            x.set_kinematics(dat.pos, dat.vel)
        x.close()
    finally:
        d.close()


# --------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def e2e_snapshot():
    n = 20000
    pos, _ = plummer(n, seed=21)
    rng = np.random.default_rng(22)
    vel = rng.normal(size=(n, 3)) * np.array([1.0, 0.8, 0.6]) + np.array([0.2, 0.0, -0.1])
    mass = rng.uniform(0.5, 1.5, n)
    sim = SimSnap({"pos": pos, "vel": vel, "mass": mass},
                  families={"dm": slice(0, 12000), "star": slice(12000, n)},
                  units_map={"pos": "kpc", "vel": "km s**-1", "mass": "Msol"})
    return sim, pos, vel, mass


def host_statistic(prof, key, arr, w):
    """The reference's per-bin loop (proarray.py:272-334) on host arrays."""
    calc = ProfileArray.get_statistic(key)
    out = np.full(prof.nbins, np.nan)
    for i, ind in enumerate(prof.binind):
        if len(ind):
            out[i] = calc(arr[ind], None if w is None else w[ind])
    return out


def check_profile(prof, fields, w, pending):
    sub = prof.sim
    if pending:
        assert all(is_pending(sub, f) for f in KINEMATIC_FIELDS)
    nb = prof.nbins
    assert np.all(np.asarray(prof.npart_bins) > 0)
    for f, key in (("vr", "mean"), ("vphi", "rms"), ("vr", "median"), ("vtheta", "mean")):
        got = np.asarray(prof[f] if key == "mean" else prof[f][key])
        ref = host_statistic(prof, key, fields[f], w)
        print(f"{f} {key}: max rel err {np.max(np.abs(got - ref) / np.abs(ref)):.2e}")
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, err_msg=f"{f} {key}")
    # dispersion: 1e-13 x the conditioning of E[x²] - E[x]²
    got = np.asarray(prof["vr"]["disp"])
    ref = host_statistic(prof, "disp", fields["vr"], w)
    sq = host_statistic(prof, "rms", fields["vr"], w) ** 2
    cond = np.maximum(1.0, sq / np.maximum(ref ** 2, 1e-300))
    assert np.all(np.abs(got - ref) / np.abs(ref) <= 1e-13 * cond + 1e-12)
    # beta = 1 - (a² + b²) / (2 c²) of three rms values, each within 1e-12
    # relative: the quotient moves by at most 4e-12 of itself (two squares
    # above, one below), then a few roundings of the expression itself
    rms = {f: host_statistic(prof, "rms", fields[f], w) for f in ("vr", "vtheta", "vphi")}
    ref = 1 - (rms["vphi"] ** 2 + rms["vtheta"] ** 2) / (2 * rms["vr"] ** 2)
    got = np.asarray(prof["beta"])
    assert got.shape == (nb,)
    tol = 4e-12 * np.abs(1 - ref) + 4 * np.finfo(float).eps * (1 + np.abs(1 - ref))
    print(f"beta: max err / tol {np.max(np.abs(got - ref) / tol):.2e}")
    assert np.all(np.abs(got - ref) <= tol)
    assert str(prof["vr"].units) == str(sub["vx"].units)
    if pending:  # no column reached the host
        assert all(is_pending(sub, f) for f in ("vr", "vtheta", "vphi"))


@pytest.mark.parametrize("weight", ["mass", None])
def test_profile_statistics_behind_a_filter(gpu, weight):
    sim, pos, vel, mass = e2e_snapshot()
    prof = RadialProfileBuilder(ndim=3, weight=weight, bins_type="equaln", nbins=32).filter(
        Sphere(4.0, cen=(0.3, -0.2, 0.1)) & FamilyFilter("dm"))(sim)
    mask = pr.sphere_mask(pos, 4.0, (0.3, -0.2, 0.1))
    mask[12000:] = False
    idx = np.nonzero(mask)[0]
    assert np.array_equal(prof.sim.get_index_list(sim), idx)
    allf = reference_fields(pos, vel)
    fields = {f: v[idx] for f, v in allf.items()}
    check_profile(prof, fields, mass[idx] if weight else None, pending=True)
    assert prof.bins._device.has_kinematics  # registered once, lazily
    # the per-particle read of the view: the kept particles' values, from the device
    assert np.array_equal(np.asarray(prof.sim["vt"]), fields["vt"], equal_nan=True)
    assert not is_pending(prof.sim, "vt") and is_pending(prof.sim, "vr")
    assert np.array_equal(np.asarray(prof.sim["vr"]), fields["vr"], equal_nan=True)


def test_profile_statistics_unfiltered(gpu):
    sim, pos, vel, mass = e2e_snapshot()
    prof = RadialProfileBuilder(ndim=3, weight="mass", bins_type="equaln", nbins=32)(sim)
    assert len(prof.sim) == len(pos)
    check_profile(prof, reference_fields(pos, vel), mass, pending=False)
    assert prof.bins._device.has_kinematics  # identity indices over the root snapshot


def test_stored_user_array_takes_the_host_route(gpu):
    _, pos, vel, mass = e2e_snapshot()
    mine = np.linspace(-1.0, 1.0, len(pos))
    sim = SimSnap({"pos": pos, "vel": vel, "mass": mass, "vr": mine}, families={"dm": slice(0, 12000)})
    prof = RadialProfileBuilder(ndim=3, weight="mass", bins_type="equaln", nbins=16).filter(
        Sphere(4.0) & FamilyFilter("dm"))(sim)
    idx = prof.sim.get_index_list(sim)
    ref = host_statistic(prof, "mean", mine[idx], mass[idx])
    np.testing.assert_allclose(np.asarray(prof["vr"]), ref, rtol=1e-12, atol=1e-15)
    assert np.array_equal(np.asarray(prof.sim["vr"]), mine[idx])
