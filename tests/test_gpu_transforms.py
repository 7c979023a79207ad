"""Frame transforms on the device: the frame rides along in the passes.

The yardstick is the library itself on rewritten arrays: a pass with a frame
must give, bit for bit, what the same pass gives on ``Frame.apply`` output
(the numpy restatement of include/pbx.h, pbx_profile_set_frame) — the
per-particle terms are then the same bits and the order of summation depends
on the particle count alone.  The frame-less passes are checked against
numpy / the oracle by tests/test_gpu_properties.py, test_gpu_kinematics.py
and test_gpu_profile.py; the sums are checked here once more against
extended-precision numpy within the project's bound, 1e-13 x the sum of
|term|.
"""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _transforms_data as td
from oracle import profile_ref as pr
from pynbodyext import _native as nat
from pynbodyext.filters import FamilyFilter, Sphere
from pynbodyext.frame import Frame, FrameView
from pynbodyext.profiles import RadialProfileBuilder
from pynbodyext.profiles._device import (ALL_COLS, KINEMATIC_FIELDS, NMOM, SRC_KIN, SRC_NONE, SRC_W,
                                         DeviceBins)
from pynbodyext.properties import KappaRot
from pynbodyext.properties import _device as pdev
from pynbodyext.synthetic import plummer
from test_gpu_kinematics import check_sums as check_bin_sums
from test_gpu_kinematics import reference_fields
from test_gpu_properties import reference_terms

pytestmark = pytest.mark.gpu
CHILD = Path(__file__).resolve().parent / "_transforms_child.py"

C = np.array([0.3, -0.2, 0.1])
VC = np.array([0.05, 0.4, -0.25])
ROT = td.euler_matrix(0.4, -0.9, 1.7)
FRAMES = {"pos": Frame(c=C), "vel": Frame(vc=VC), "rot": Frame(R=ROT), "all": Frame(C, VC, ROT)}
SPHERE = ((0.1, -0.05, 0.02), 1.5)  # in frame coordinates
WINDOW = {"bin_min": 1e-3, "bin_max": 60.0}  # (keeps a NaN x out of the equaln edges)

# one sweep of the property pass's full grid (csrc/property.hip: 1024 blocks x
# 256 threads x 4 particles); 1000 more start a second sweep
SWEEP = 1024 * 256 * 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def particles(n):
    """(pos, vel, mass, family ranges whose span starts at a non-zero base)."""
    if n == 1:
        pos = np.array([[0.6, -0.7, 1.1]])
    else:
        pos, _ = plummer(n, seed=40 + n % 97)
    pos = pos + C
    rng = np.random.default_rng(n)
    vel = rng.normal(size=(n, 3)) + VC
    mass = rng.uniform(0.5, 1.5, n)
    fams = None if n < 8 else [(n // 8 + 1, n // 2), (n // 2 + 3, n - n // 10)]
    return pos, vel, mass, fams


# ------------------------------------------------- 1. the property pass
@pytest.mark.parametrize("which", sorted(FRAMES))
@pytest.mark.parametrize("n", [1, 63, 1025, 5000, SWEEP + 1000])
def test_property_moments_frame_bit_identical(gpu, n, which):
    pos, vel, mass, fams = particles(n)
    fr = FRAMES[which]
    fpos, fvel = fr.pos(pos), fr.vel(vel)
    for sphere in (None, SPHERE):
        for families in ((None, fams) if fams else (None,)):
            got = pdev.moments(pos, vel, mass, groups=pdev.ALL_GROUPS, sphere=sphere,
                               families=families, frame=fr)
            ref = pdev.moments(fpos, fvel, mass, groups=pdev.ALL_GROUPS, sphere=sphere,
                               families=families)
            what = (n, which, sphere is not None, families is not None)
            assert got[0] == ref[0], what
            assert same_bits(got[1], ref[1]), (what, got[1], ref[1])
            if sphere is not None and n >= 63:
                assert 0 < got[0] < n
    # a group that reads one array only: the other half of the frame changes nothing
    for groups in (pdev.MASS | pdev.COM, pdev.COV, pdev.MASS):
        got = pdev.moments(pos, vel, mass, groups=groups, sphere=SPHERE, frame=fr)
        ref = pdev.moments(fpos, fvel, mass, groups=groups, sphere=SPHERE)
        assert got[0] == ref[0] and same_bits(got[1], ref[1]), (n, which, groups)


@pytest.mark.parametrize("n", [5000, SWEEP + 1000])
def test_property_moments_frame_against_extended_precision(gpu, n):
    pos, vel, mass, fams = particles(n)
    fr = FRAMES["all"]
    fpos, fvel = fr.pos(pos), fr.vel(vel)
    keep = pr.sphere_mask(fpos, SPHERE[1], SPHERE[0])
    fam = np.zeros(n, dtype=bool)
    for a, b in fams:
        fam[a:b] = True
    keep &= fam
    n_kept, sums = pdev.moments(pos, vel, mass, groups=pdev.ALL_GROUPS, sphere=SPHERE,
                                families=fams, frame=fr)
    assert n_kept == int(keep.sum()) and n_kept > 100
    for j, row in enumerate(reference_terms(fpos[keep], fvel[keep], mass[keep])):
        tl = row.astype(np.longdouble)
        err, mag = abs(np.longdouble(sums[j]) - tl.sum()), np.abs(tl).sum()
        print(f"n={n} sum {j}: err / Σ|term| = {float(err / mag):.2e}")
        assert err <= np.longdouble(1e-13) * mag, (n, j)


def test_property_frame_unkept_and_infinite_particles(gpu):
    pos, vel, mass, fams = (a.copy() if isinstance(a, np.ndarray) else a for a in particles(5000))
    fr = FRAMES["all"]
    out_fam = fams[0][1] + 1  # in the gap between the family ranges
    fpos = fr.pos(pos)
    out_sph = int(np.nonzero(~pr.sphere_mask(fpos, SPHERE[1], SPHERE[0])[fams[0][0]:fams[0][1]])[0][0]) \
        + fams[0][0]
    clean = pdev.moments(pos, vel, mass, groups=pdev.ALL_GROUPS, sphere=SPHERE, families=fams, frame=fr)
    pos[out_fam], vel[out_fam], mass[out_fam] = np.inf, np.nan, np.nan
    pos[out_sph] = [np.inf, -np.inf, np.nan]  # (inf through the rotation is NaN: still not kept)
    vel[out_sph] = np.inf
    dirty = pdev.moments(pos, vel, mass, groups=pdev.ALL_GROUPS, sphere=SPHERE, families=fams, frame=fr)
    assert dirty[0] == clean[0] and same_bits(dirty[1], clean[1])
    assert np.all(np.isfinite(dirty[1]))
    # a kept infinity with the rotation flag off stays an infinity: the step is
    # skipped, not run with the zeros the packed frame holds for it (0 * inf)
    pos, vel, mass, _ = (a.copy() if isinstance(a, np.ndarray) else a for a in particles(63))
    pos[5, 0] = np.inf
    n_kept, sums = pdev.moments(pos, vel, mass, groups=pdev.MASS | pdev.COM | pdev.COV,
                                frame=Frame(c=C, vc=VC))
    assert n_kept == 63 and sums[1] == np.inf and np.all(np.isfinite(sums[[0, 2, 3, 4, 5, 6]]))
    ref = pdev.moments(pos - C, vel - VC, mass, groups=pdev.MASS | pdev.COM | pdev.COV)
    assert same_bits(sums, ref[1])
    with pytest.raises(ValueError, match="PBX_FRAME"):
        packed = np.zeros(15)
        kept, out = nat.c_int64(0), np.zeros(18)
        nat.call("pbx_property_moments_frame", nat.vptr(pos), nat.vptr(vel), nat.vptr(mass), 63, 0,
                 0, None, None, 0, pdev.MASS, 8, nat.dptr(packed), nat.ctypes.byref(kept),
                 nat.dptr(out))


# ------------------------------------------------ 2. the profile handle
class Pair:
    """The same selection twice: a handle with the frame over the stored
    arrays, and a frame-less handle over Frame.apply's arrays."""

    def __init__(self, n, which, kind, sphere=SPHERE, nbins=8, with_fams=True, special=True):
        pos, vel, mass, fams = particles(n)
        pos, vel = pos.copy(), vel.copy()
        self.fr = fr = FRAMES[which]
        if special and n > 100:
            pos[n // 3] = np.nan  # a NaN position (kept without a sphere, dropped by one)
            if fr.c is not None and fr.R is None:
                pos[n // 3 + 1] = fr.c  # exactly the frame's origin: 0/0 in the fields
        self.fams = fams if with_fams else None
        self.sphere, self.kind, self.n = sphere, kind, n
        self.pos, self.vel, self.mass = pos, vel, mass
        self.fpos, self.fvel = fr.pos(pos), fr.vel(vel)
        self.keep = []
        self.framed = self._make(pos, vel, fr, nbins)
        self.plain = self._make(self.fpos, self.fvel, None, nbins)

    def _make(self, pos, vel, fr, nbins):
        d = DeviceBins()
        d.set_frame(fr)
        kw = dict(sphere=self.sphere, families=self.fams)
        if self.kind == "eager":
            DeviceBins.select(pos, self.mass, into=d, frame=fr, **kw)
            d.set_kinematics(pos, vel)
            return d, None
        stats = [(SRC_W, SRC_NONE, 1 << 3)]
        try:  # (nothing kept: the reference's error, from both handles alike)
            if self.kind == "lazy":
                _, e, c, m = DeviceBins.radial_equaln(pos, self.mass, nbins=nbins, into=d,
                                                      stats=stats, **WINDOW, **kw)
                d.set_kinematics(pos, vel)
                return d, (e, c, m)
            dp, dm, dv = (nat.DeviceArray.from_host(a) for a in (pos, self.mass, vel))
            self.keep += [dp, dm, dv]
            _, e, c, m = DeviceBins.radial_equaln(dp.ptr, dm.ptr, nbins=nbins, on_device=True,
                                                  n=self.n, into=d, stats=stats, **WINDOW, **kw)
            d.set_kinematics(dp.ptr, dv.ptr, on_device=True, n=self.n)
            return d, (e, c, m)
        except (ValueError, IndexError) as err:
            return d, str(err)

    def close(self):
        for d in (self.framed[0], self.plain[0]):
            d.close()
        for a in self.keep:
            a.free()


def compare_pair(p: Pair, nbins=8, fields=True):
    (a, ra), (b, rb) = p.framed, p.plain
    what = (p.n, p.kind)
    assert a.n == b.n, what
    if isinstance(ra, str) or isinstance(rb, str):
        assert ra == rb and a.n < 2, (what, ra, rb)
        return
    if ra is not None:  # the one-call path's own edges, counts and sums
        assert same_bits(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]), what
        # (per-bin sums add with LDS float atomics: the last bits follow the
        # arrival order, run to run — test_gpu_switches' bound)
        np.testing.assert_allclose(ra[2][0], rb[2][0], rtol=1e-12, atol=0, err_msg=str(what))
    sa, sb = a.selection(), b.selection()
    assert np.array_equal(sa[0], sb[0]) and same_bits(sa[1], sb[1]) and same_bits(sa[2], sb[2]), what
    if a.n == 0:
        return
    # the numpy mask and r of the rewritten arrays
    keep = np.ones(p.n, dtype=bool)
    if p.sphere is not None:
        keep &= pr.sphere_mask(p.fpos, p.sphere[1], p.sphere[0])
    if p.fams is not None:
        fam = np.zeros(p.n, dtype=bool)
        for lo, hi in p.fams:
            fam[lo:hi] = True
        keep &= fam
    assert np.array_equal(sa[0], np.nonzero(keep)[0]), what
    assert same_bits(sa[1], pr.radial_r(p.fpos)[keep]), what
    assert same_bits(np.array(a.minmax()), np.array(b.minmax())), what  # lin / log edges' inputs
    finite = sa[1][np.isfinite(sa[1])]
    if len(finite) >= 2:
        ea, eb = a.edges_equaln(nbins, **WINDOW), b.edges_equaln(nbins, **WINDOW)
        assert same_bits(ea, eb), what
        lo, hi = float(finite.min()), float(finite.max())
        for edges in (ea, np.linspace(lo, hi, nbins + 1),
                      np.logspace(np.log10(max(lo, 1e-3)), np.log10(hi), nbins + 1)):
            if not np.all(np.diff(edges) >= 0):
                continue
            assert np.array_equal(a.assign(edges), b.assign(edges)), what
            (pa, oa), (pb, ob) = a.csr(), b.csr()
            assert np.array_equal(pa, pb) and np.array_equal(oa, ob), what
    if fields:
        for f in KINEMATIC_FIELDS:
            fa, fb = a.kinematic_field(f), b.kinematic_field(f)
            assert same_bits(fa, fb), (what, f)
            ref = reference_fields(p.fpos, p.fvel)[f][sa[0]]
            assert np.array_equal(fa, ref, equal_nan=True), (what, f)


@pytest.mark.parametrize("which", sorted(FRAMES))
@pytest.mark.parametrize("kind", ["eager", "lazy", "ondev"])
@pytest.mark.parametrize("n", [1, 4095, 4097, 20000])
def test_profile_handle_with_a_frame_bit_identical(gpu, n, kind, which):
    for sphere in (SPHERE, None):
        p = Pair(n, which, kind, sphere=sphere, with_fams=n >= 8)
        try:
            compare_pair(p)
            if sphere is None and n > 100:  # the NaN position is kept: NaN fields compared too
                assert np.isnan(p.framed[0].kinematic_field("v2")).sum() == 0
                assert np.isnan(p.framed[0].kinematic_field("vr")).sum() >= 1
        finally:
            p.close()


@pytest.mark.parametrize("nbins,weighted", [(8, True), (128, False), (200, True)])
def test_kinematic_sums_in_a_frame(gpu, nbins, weighted):
    """The fused and the generic sums (200 bins: the fused call's own
    fallback) against extended precision, test_gpu_kinematics' bound."""
    p = Pair(20000, "all", "eager", special=False)
    try:
        d = p.framed[0]
        idx, x, w = d.selection()
        edges = d.edges_equaln(nbins)
        assert same_bits(edges, pr.edges_equaln(x, nbins))
        d.assign(edges)
        b = pr.bin_ids(x, edges)
        wsrc, wv = (SRC_W, w) if weighted else (SRC_NONE, None)
        fused = d.kinematic_moments(KINEMATIC_FIELDS, wsrc, ALL_COLS)
        assert fused.shape == (6, nbins, NMOM)
        ref = reference_fields(p.fpos, p.fvel)
        for k, f in enumerate(KINEMATIC_FIELDS):
            vals = ref[f][idx]
            mag = check_bin_sums(fused[k], vals, wv, b, nbins, f"fused {f}")
            generic = d.moments(SRC_KIN(f), wsrc, ALL_COLS)
            check_bin_sums(generic, vals, wv, b, nbins, f"generic {f}")
            assert np.all(np.abs(fused[k] - generic) <= 1e-13 * mag), f
    finally:
        p.close()


def test_lazy_tiled_selection_with_a_frame(gpu):
    """4,194,304 + 5 particles: 1025 selection tiles, the tiled lazy path.
    Three calls per handle, so the hinted and the speculating variants run;
    a speculating call keeps no x and rebuilds it from the positions — in the
    frame — for the reader below."""
    n = 4_194_304 + 5
    rng = np.random.default_rng(9)
    pos = rng.normal(scale=3.0, size=(n, 3)) + C
    mass = rng.uniform(0.5, 1.5, n)
    fr = FRAMES["all"]
    fpos = fr.pos(pos)
    stats = [(SRC_W, SRC_NONE, 1 << 3)]
    out = []
    for arr, frame in ((pos, fr), (fpos, None)):
        d = DeviceBins()
        d.set_frame(frame)
        dp, dm = nat.DeviceArray.from_host(arr), nat.DeviceArray.from_host(mass)
        d.set_source_stable(True)
        try:
            calls = []
            for _ in range(3):
                _, e, c, m = DeviceBins.radial_equaln(dp.ptr, dm.ptr, nbins=128, sphere=((0.0, 0.0, 0.0), 9.0),
                                                      on_device=True, n=n, into=d, stats=stats,
                                                      bin_min=0.3, bin_max=8.0)
                calls.append((e, c, m[0], d.csr()))
            out.append((calls, d.selection(), d.level0_stats(), d.spec_stats()))
        finally:
            d.close()
            dp.free()
            dm.free()
    (ca, sa, la, pa), (cb, sb, lb, pb) = out
    assert la["tiled"] == 3 and la == lb and pa == pb, (la, lb, pa, pb)
    for (ea, na, ma, (perm_a, off_a)), (eb, nb_, mb, (perm_b, off_b)) in zip(ca, cb):
        assert same_bits(ea, eb) and np.array_equal(na, nb_)
        assert np.array_equal(perm_a, perm_b) and np.array_equal(off_a, off_b)
        np.testing.assert_allclose(ma, mb, rtol=1e-12, atol=0)  # (float atomics: test_gpu_switches)
    assert np.array_equal(sa[0], sb[0]) and same_bits(sa[1], sb[1]) and same_bits(sa[2], sb[2])
    keep = pr.sphere_mask(fpos, 9.0)
    assert np.array_equal(sa[0], np.nonzero(keep)[0]) and same_bits(sa[1], pr.radial_r(fpos)[keep])


@pytest.mark.parametrize("group", ["timing", "traces", "precise"])
def test_frame_under_the_runtime_switches(gpu, tmp_path, group):
    """The 20000 case under every runtime variable tests/test_gpu_switches.py
    switches (they are read once per process: a child runs the comparison of
    this file's Pair, framed handle against rewritten arrays, and fails on
    the first difference)."""
    extra = {"timing": {"GRAVITY_TIMING": "1"},
             "traces": {"PBX_MONO_TRACE": "1", "PBX_WALK_TRACE": f"{tmp_path}/walk_trace.bin"},
             "precise": {"PBX_PRECISE": "1"}}[group]
    env = {k: v for k, v in os.environ.items()
           if not (k.startswith("PBX_") or k == "GRAVITY_TIMING") or k == "PBX_LIBRARY"}
    env.update(extra)
    r = subprocess.run([sys.executable, str(CHILD)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, f"{group}: rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert "frame pairs identical" in r.stdout
    if group == "timing":
        assert "pbx." in r.stderr
    if group == "traces":
        assert "[mono]" in r.stderr


# ----------------------------------------------- 3. life cycle and errors
def test_frame_life_cycle_and_errors(gpu):
    pos, vel, mass, fams = particles(4097)
    fr = FRAMES["all"]
    fpos = fr.pos(pos)
    d = DeviceBins()
    try:
        d.set_frame(fr)
        want = pr.radial_r(fpos)[pr.sphere_mask(fpos, SPHERE[1], SPHERE[0])]
        for _ in range(2):  # the frame survives a second selection (no frame argument given)
            kept = nat.c_int64(0)
            args, keep = DeviceBins._select_args(pos, mass, SPHERE, None, 3, False, None)
            nat.call("pbx_profile_select", d._h, *args, nat.ctypes.byref(kept))
            d.n, d.has_selection = kept.value, True
            assert same_bits(d.selection()[1], want)
        # float32 positions with a frame set: an argument error (the host route's case)
        with pytest.raises(ValueError, match="frame is set"):
            DeviceBins.select(pos.astype(np.float32), mass, into=d, frame=fr)
        with pytest.raises(ValueError, match="PBX_FRAME"):
            nat.call("pbx_profile_set_frame", d._h, 8, nat.dptr(fr.packed()))
        # cleared by NULL: the stored coordinates again
        nat.call("pbx_profile_set_frame", d._h, 7, None)
        d._frame = None
        DeviceBins.select(pos, mass, sphere=SPHERE, into=d)
        assert same_bits(d.selection()[1], pr.radial_r(pos)[pr.sphere_mask(pos, SPHERE[1], SPHERE[0])])
        DeviceBins.select(pos.astype(np.float32), mass, into=d)  # and float32 is accepted again
        # select(frame=None) on a reused handle clears an earlier frame as well
        DeviceBins.select(pos, mass, sphere=SPHERE, into=d, frame=fr)
        assert same_bits(d.selection()[1], want)
        DeviceBins.select(pos, mass, sphere=SPHERE, into=d)
        assert same_bits(d.selection()[1], pr.radial_r(pos)[pr.sphere_mask(pos, SPHERE[1], SPHERE[0])])
    finally:
        d.close()


# ------------------------------------------------------- 4. the public API
@pytest.fixture(scope="module")
def disc():
    pos, vel, mass = td.disc_arrays()
    mpos, mvel = td.moved(pos, vel)
    return td.snapshot(mpos, mvel, mass), (pos, vel, mass)


def test_larger_example_runs_fused_and_equals_the_materialised_route(gpu, disc):
    sim, _ = disc
    before = {k: np.asarray(sim[k]).tobytes() for k in ("pos", "vel", "mass")}
    res = td.example().run(sim, perf_time=True)
    for cls in ("CenPos", "ParamContain", "CenVel", "AngMomVec", "KappaRot"):
        # every property took its device route, none the numpy calculate
        assert f"{cls}.device" in res.perf and f"{cls}.calculate" not in res.perf, \
            (cls, sorted(res.perf))
    framed = td.example_transform()(sim)
    assert isinstance(framed, FrameView) and framed._frame.flags == 7 and framed._frame_base is sim
    assert not framed._derived  # nothing rewrote pos / vel on the host
    mat = framed._frame.apply(sim)  # the materialised route: rewritten arrays, no frame
    assert res.value == KappaRot().filter(td.example_scope())(mat)
    assert all(np.asarray(sim[k]).tobytes() == b for k, b in before.items())

    # the profile: binning and every per-particle field, device-held or host
    builder = RadialProfileBuilder(weight="mass", bins_type="equaln", nbins=16)
    prof = builder.filter(td.example_scope()).transform(td.example_transform())(sim)
    ref = builder.filter(td.example_scope())(mat)
    assert same_bits(np.asarray(prof.bin_edges), np.asarray(ref.bin_edges))
    assert np.array_equal(prof.npart_bins, ref.npart_bins)
    assert all(np.array_equal(a, b) for a, b in zip(prof.binind, ref.binind))
    root = prof.sim.ancestor
    assert isinstance(root, FrameView) and root._frame_base is sim
    for key in ("r", "mass", "vr", "vphi", "vtheta"):  # read from the device: no host frame built
        assert same_bits(np.asarray(prof.sim[key]), np.asarray(ref.sim[key])), key
    assert not root._derived
    # a host field is the frame's, computed on demand; other arrays pass through
    assert same_bits(np.asarray(prof.sim["vx"]), np.asarray(ref.sim["vx"])) and "vel" in root._derived
    assert "pos" not in root._derived
    assert np.array_equal(prof.particles_at_bin[3]["pos"], ref.particles_at_bin[3]["pos"])
    assert np.array_equal(prof.star.npart_bins, ref.star.npart_bins)
    assert same_bits(np.asarray(prof.star.sim["vy"]), np.asarray(ref.star.sim["vy"]))
    assert all(np.asarray(sim[k]).tobytes() == b for k, b in before.items())


def test_larger_example_profile_statistics_equal_the_materialised_route(gpu, disc):
    """["vphi"], ["vr"]["disp"] and ["beta"] of the profile built in the frame
    against the same builder on the materialised snapshot, bit for bit.

    The selection, the edges, the bin of every particle and the per-particle
    fields are bit-identical (the test above), so the statistics are as soon
    as the per-bin sums add their terms in a fixed order.  They do: no two
    waves of a block add into the same LDS accumulator at once (a copy per
    wave, or turns: moments_kernel, kin_moments_kernel), and the waves' copies
    and the blocks' rows are reduced in a fixed order.
    With all waves adding at once the last bits moved from call to call (up
    to 5e-16 relative, also between two builds of the materialised profile),
    so the yardstick's own repeatability is asserted beside the comparison."""
    sim, _ = disc
    framed = td.example_transform()(sim)
    mat = framed._frame.apply(sim)
    builder = RadialProfileBuilder(weight="mass", bins_type="equaln", nbins=16)
    prof = builder.filter(td.example_scope()).transform(td.example_transform())(sim)
    ref = builder.filter(td.example_scope())(mat)
    again = builder.filter(td.example_scope())(mat)
    same = []
    for name, pick in (("vphi", lambda p: p["vphi"]), ("vr disp", lambda p: p["vr"]["disp"]),
                       ("beta", lambda p: p["beta"]), ("vphi rms", lambda p: p["vphi"]["rms"]),
                       ("mass sum", lambda p: p["mass"]["sum"])):
        got, want, rep = (np.asarray(pick(p), dtype=np.float64) for p in (prof, ref, again))
        print(f"{name}: framed vs materialised max rel {float(np.max(np.abs(got - want) / np.abs(want))):.2e}"
              f"; materialised vs materialised again {float(np.max(np.abs(rep - want) / np.abs(want))):.2e}")
        same.append((name, same_bits(got, want), same_bits(rep, want)))
    assert all(a and b for _, a, b in same), same


def test_larger_example_recovers_the_unrotated_disc(gpu, disc):
    """kappa_rot of the rotated, displaced and boosted disc through the
    example against the disc's own (the example by hand in longdouble on the
    unmoved arrays: 0.97101581116669732).  The routes do not agree to
    rounding: the shrinking sphere starts from the snapshot's x extent, which
    the rotation changes.  The host route deviates by 1.302e-05 on this input
    (measured on the CPU, float64 host route against the longdouble value);
    the tolerance is 10 x that."""
    sim, _ = disc
    got = td.example()(sim)
    print(f"kappa_rot {got!r}: deviation {abs(got - 0.97101581116669732):.3e}")
    assert abs(got - 0.97101581116669732) <= 10 * 1.302e-05
    assert got > 0.9  # a cold disc seen face-on; edge-on it is far lower
    assert KappaRot().filter(Sphere(30.0, cen=td.SHIFT) & FamilyFilter("star"))(sim) < 0.6
