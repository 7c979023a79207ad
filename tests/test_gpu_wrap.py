"""The periodic wrap of the frame on the device, and WrapBox end to end.

The yardstick is that of tests/test_gpu_transforms.py: a pass with the frame
must give, bit for bit, what the same pass gives on ``Frame.apply`` output
(the numpy statement of include/pbx.h, which tests/test_wrap_cpu.py pins to
the reference's own bits).  The wrap sits between the shift and the rotation.
"""
import functools
from pathlib import Path

import numpy as np
import pytest

import _transforms_data as td
from pynbodyext import _native as nat
from pynbodyext.filters import FamilyFilter, Sphere
from pynbodyext.frame import Frame, FrameView, choose_lower, wrap_extents
from pynbodyext.profiles import RadialProfileBuilder
from pynbodyext.profiles._device import ALL_COLS, KINEMATIC_FIELDS, SRC_W, DeviceBins
from pynbodyext.properties import KappaRot, ParamContain
from pynbodyext.properties import _device as pdev
from pynbodyext.simcore import SimSnap
from pynbodyext.synthetic import plummer
from pynbodyext.transforms import ShiftPosTo
from pynbodyext.transforms.wrap import WrapBox
from test_gpu_kinematics import reference_fields

pytestmark = pytest.mark.gpu

L = 25.0 / 0.7  # not a power of two
CENTRE = np.array([L - 0.4, 0.3, L - 0.2])  # near a box corner
VC = np.array([0.05, 0.4, -0.25])
ROT = td.euler_matrix(0.4, -0.9, 1.7)
CENTER_LO, UPPER_LO = np.full(3, -0.5 * L), np.zeros(3)
FRAMES = {
    "center": Frame(wrap=(L, CENTER_LO)),
    "upper": Frame(wrap=(L, UPPER_LO)),
    "mixed": Frame(wrap=(L, np.array([-0.5 * L, 0.0, -0.5 * L]))),
    "shift": Frame(CENTRE, wrap=(L, CENTER_LO)),
    "shift_rot": Frame(CENTRE, None, ROT, (L, CENTER_LO)),
    "all": Frame(CENTRE, VC, ROT, (L, CENTER_LO)),
}
SPHERE = ((0.1, -0.05, 0.02), 1.5)  # in frame coordinates
# one sweep of the property pass's full grid (csrc/property.hip); 1000 more
# start a second sweep
SWEEP = 1024 * 256 * 4


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(bits(x), bits(y))


def same_values(x, y):
    """Bit-equal where finite or infinite, NaN at the same places."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    nan = np.isnan(x)
    return x.shape == y.shape and np.array_equal(nan, np.isnan(y)) and \
        np.array_equal(bits(x[~nan]), bits(y[~nan]))


@functools.lru_cache(maxsize=None)
def particles(n):
    """A Plummer sphere around CENTRE reduced into [0, L): (pos, vel, mass,
    family ranges whose span starts at a non-zero base)."""
    if n == 1:
        off = np.array([[0.6, -0.7, 1.1]])
    else:
        off, _ = plummer(n, seed=140 + n % 97)
    pos = np.mod(CENTRE + off, L)
    assert pos.min() >= 0.0 and pos.max() < L
    rng = np.random.default_rng(n)
    vel = rng.normal(size=(n, 3)) + VC
    mass = rng.uniform(0.5, 1.5, n)
    fams = None if n < 8 else [(n // 8 + 1, n // 2), (n // 2 + 3, n - n // 10)]
    return pos, vel, mass, fams


@functools.lru_cache(maxsize=None)
def raw_particles(n):
    """The same sphere (its tail reaches 50 > L) left where it is: not reduced."""
    off, _ = plummer(n, seed=140 + n % 97)
    return CENTRE + off


def test_the_cloud_crosses_every_face():
    """A cloud reduced into [0, L) spans one box length, so after the shift
    to its centre an axis holds two values of k, not three: k = -1 and 0 where
    the centre is near the upper face (x, z), 0 and 1 near the lower one (y).
    The unreduced cloud holds k = -1, 0 and 1 on every axis; the moments test
    runs on both."""
    pos = particles(5000)[0]
    k = np.floor((pos - CENTRE + 0.5 * L) / L)
    assert [sorted(set(k[:, axis])) for axis in range(3)] == [[-1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]]
    k = np.floor((raw_particles(5000) - CENTRE + 0.5 * L) / L)
    for axis in range(3):
        assert {-1.0, 0.0, 1.0} <= set(k[:, axis]), axis


# ------------------------------------------------- 1. the property passes
@pytest.mark.parametrize("which", sorted(FRAMES))
@pytest.mark.parametrize("n", [1, 63, 1025, 5000, SWEEP + 1000])
def test_moments_with_a_wrap_bit_identical(gpu, n, which):
    pos, vel, mass, fams = particles(n)
    fr = FRAMES[which]
    fpos, fvel = fr.pos(pos), fr.vel(vel)
    kept = []
    for sphere in (None, SPHERE):
        for families in ((None, fams) if fams else (None,)):
            got = pdev.moments(pos, vel, mass, groups=pdev.ALL_GROUPS, sphere=sphere,
                               families=families, frame=fr)
            ref = pdev.moments(fpos, fvel, mass, groups=pdev.ALL_GROUPS, sphere=sphere,
                               families=families)
            what = (n, which, sphere is not None, families is not None)
            assert got[0] == ref[0], what
            assert same_bits(got[1], ref[1]), (what, got[1], ref[1])
            kept.append(got[0])
    if n >= 1025 and which in ("center", "shift", "shift_rot", "all"):
        assert 0 < kept[2] < n  # (the sphere holds the whole halo's core)
    if n in (63, 5000):  # the unreduced cloud: k = -1, 0, 1 (and 2) on every axis
        raw = raw_particles(n)
        got = pdev.moments(raw, vel, mass, groups=pdev.ALL_GROUPS, sphere=SPHERE, families=fams,
                           frame=fr)
        ref = pdev.moments(fr.pos(raw), fvel, mass, groups=pdev.ALL_GROUPS, sphere=SPHERE,
                           families=fams)
        assert got[0] == ref[0] and same_bits(got[1], ref[1]), (n, which, "unreduced")
    # the wrap-less frame gives other sums: the wrap is not ignored
    if n >= 63 and which == "shift":
        with_wrap = pdev.moments(pos, vel, mass, groups=pdev.ALL_GROUPS, frame=fr)
        without = pdev.moments(pos, vel, mass, groups=pdev.ALL_GROUPS, frame=Frame(CENTRE))
        assert not same_bits(with_wrap[1], without[1])


@pytest.mark.parametrize("which", sorted(FRAMES))
@pytest.mark.parametrize("n", [63, 5000, SWEEP + 1000])
def test_enclosed_and_virial_radius_with_a_wrap(gpu, n, which):
    pos, _, mass, fams = particles(n)
    fr = FRAMES[which]
    fpos = fr.pos(pos)
    t = np.array([0.0, 0.25, 0.5, 1.0, 2.0, 0.5 * L, L, np.inf, np.nan])
    for scope in ({}, {"sphere": SPHERE, "families": fams}):
        got = pdev.enclosed(pos, mass, t, frame=fr, **scope)
        ref = pdev.enclosed(fpos, mass, t, **scope)
        what = (n, which, sorted(scope))
        assert got[0] == ref[0] and np.array_equal(got[2], ref[2]), what
        assert same_bits(got[1], ref[1]), what
        assert same_values(got[3], ref[3]), (what, got[3], ref[3])
    r = np.sqrt((fpos[:, 0] * fpos[:, 0] + fpos[:, 1] * fpos[:, 1]) + fpos[:, 2] * fpos[:, 2])
    target = float(mass[r < 1.0].sum() / (4.0 * np.pi / 3.0)) if (r < 1.0).any() else 1.0
    got = pdev.virial_radius(pos, mass, target_rho=target, eta=1e-3 * target, frame=fr)
    ref = pdev.virial_radius(fpos, mass, target_rho=target, eta=1e-3 * target)
    assert same_values(got[0], ref[0]) and got[1:] == ref[1:], (n, which, got, ref)
    if which in ("shift", "center") and n > SWEEP:
        assert got[4] and 0.5 < got[0] < 2.0  # (the whole halo: the radius is near 1)


# ------------------------------------------------- 2. the profile handle
@pytest.mark.parametrize("which", sorted(FRAMES))
@pytest.mark.parametrize("n", [63, 5000])
def test_selection_and_kinematics_with_a_wrap(gpu, n, which):
    pos, vel, mass, fams = particles(n)
    fr = FRAMES[which]
    fpos, fvel = fr.pos(pos), fr.vel(vel)
    for sphere in (SPHERE, None):
        framed = DeviceBins.select(pos, mass, sphere=sphere, families=fams, frame=fr)
        plain = DeviceBins.select(fpos, mass, sphere=sphere, families=fams)
        try:
            framed.set_kinematics(pos, vel)
            plain.set_kinematics(fpos, fvel)
            sa, sb = framed.selection(), plain.selection()
            what = (n, which, sphere is not None)
            assert np.array_equal(sa[0], sb[0]) and same_bits(sa[1], sb[1]), what
            assert same_bits(sa[2], sb[2]), what
            # numpy on the host statement
            keep = np.zeros(n, dtype=bool)
            for lo, hi in fams:
                keep[lo:hi] = True
            r = np.sqrt((fpos[:, 0] * fpos[:, 0] + fpos[:, 1] * fpos[:, 1])
                        + fpos[:, 2] * fpos[:, 2])
            if sphere is not None:
                d = fpos - np.asarray(sphere[0])
                keep &= ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) \
                    < sphere[1] * sphere[1]
            assert np.array_equal(sa[0], np.nonzero(keep)[0]) and same_bits(sa[1], r[keep]), what
            if framed.n == 0:
                continue
            ref = reference_fields(fpos, fvel)
            for f in KINEMATIC_FIELDS:
                fa, fb = framed.kinematic_field(f), plain.kinematic_field(f)
                assert same_values(fa, fb), (what, f)
                assert same_values(fa, ref[f][sa[0]]), (what, f)
            if framed.n >= 16:
                edges = framed.edges_equaln(4)
                assert same_bits(edges, plain.edges_equaln(4)), what
                assert np.array_equal(framed.assign(edges), plain.assign(edges)), what
                ka = framed.kinematic_moments(KINEMATIC_FIELDS, SRC_W, ALL_COLS)
                kb = plain.kinematic_moments(KINEMATIC_FIELDS, SRC_W, ALL_COLS)
                assert same_values(ka, kb), what
        finally:
            framed.close()
            plain.close()


def test_lazy_tiled_selection_with_a_wrap(gpu):
    """4,194,304 + 5 particles: 1025 selection tiles, the tiled lazy path of
    tests/test_gpu_transforms.py, with a wrap in the frame.  Five identical
    calls per handle, so the hinted variants run and a handle may speculate
    (tests/test_gpu_profile.py: from the fourth call on).  A speculating call
    keeps no x and rebuilds it from the positions with the wrap-less code, so
    a handle whose frame holds a wrap must not speculate; the reader below
    gets the x it stored."""
    n = 4_194_304 + 5
    rng = np.random.default_rng(19)
    pos = np.mod(CENTRE + rng.normal(scale=3.0, size=(n, 3)), L)
    mass = rng.uniform(0.5, 1.5, n)
    fr = FRAMES["shift_rot"]
    fpos = fr.pos(pos)
    stats = [(SRC_W, -1, 1 << 3)]
    out = []
    for arr, frame in ((pos, fr), (fpos, None)):
        d = DeviceBins()
        d.set_frame(frame)
        dp, dm = nat.DeviceArray.from_host(arr), nat.DeviceArray.from_host(mass)
        d.set_source_stable(True)
        try:
            calls = []
            for _ in range(5):
                _, e, c, m = DeviceBins.radial_equaln(dp.ptr, dm.ptr, nbins=128,
                                                      sphere=((0.0, 0.0, 0.0), 9.0), on_device=True,
                                                      n=n, into=d, stats=stats, bin_min=0.3,
                                                      bin_max=8.0)
                calls.append((e, c, d.csr()))
            out.append((calls, d.selection(), d.level0_stats(), d.spec_stats()))
        finally:
            d.close()
            dp.free()
            dm.free()
    (ca, sa, la, pa), (cb, sb, lb, pb) = out
    print(f"level0 {la} / {lb}; speculation with a wrap {pa}, on rewritten arrays {pb}")
    assert la["tiled"] == 5 and lb["tiled"] == 5, (la, lb)
    assert not any(pa.values()), pa  # (a wrap frame never speculates)
    for (ea, na, (perm_a, off_a)), (eb, nb_, (perm_b, off_b)) in zip(ca, cb):
        assert same_bits(ea, eb) and np.array_equal(na, nb_)
        assert np.array_equal(perm_a, perm_b) and np.array_equal(off_a, off_b)
    assert np.array_equal(sa[0], sb[0]) and same_bits(sa[1], sb[1]) and same_bits(sa[2], sb[2])
    r2 = (fpos[:, 0] * fpos[:, 0] + fpos[:, 1] * fpos[:, 1]) + fpos[:, 2] * fpos[:, 2]
    keep = r2 < 81.0
    assert np.array_equal(sa[0], np.nonzero(keep)[0]) and same_bits(sa[1], np.sqrt(r2)[keep])
    assert keep.sum() > 0.9 * n  # (the halo is whole: without the wrap an eighth of it is kept)


def test_planted_rows_keep_the_reference_bits(gpu):
    """-0.0, exact multiples of L and the half-box points through the device's
    wrap: the one place where the compiler could fold the "+ 0.0" away.  With
    y' = 1, v = (0, 1, 0): vphi = (x'*1 - 1*0) / rxy carries the sign of x',
    the sign of a zero included."""
    gold = np.load(Path(__file__).resolve().parent / "golden" / "wrapbox.npz")
    for box in (7.123456789, 100.0, L):
        edge = np.array([0.0, -0.0, box, -box, 0.5 * box, -0.5 * box, np.nextafter(0.5 * box, 0),
                         2.0 * box, -3.0 * box, np.nextafter(-0.5 * box, 0)])
        n = len(edge)
        pos = np.zeros((3 * n, 3))
        vel = np.zeros((3 * n, 3))
        for axis in range(3):  # the planted values on one axis, 1.0 and 0.25 on the others
            rows = slice(axis * n, (axis + 1) * n)
            pos[rows, axis] = edge
            pos[rows, (axis + 1) % 3] = 1.0
            pos[rows, (axis + 2) % 3] = 0.25
            vel[rows, (axis + 1) % 3] = 1.0
        mass = np.ones(3 * n)
        for lo in (np.full(3, -0.5 * box), np.zeros(3)):
            fr = Frame(wrap=(box, lo))
            fpos = fr.pos(pos)
            d = DeviceBins.select(pos, mass, frame=fr)
            try:
                d.set_kinematics(pos, vel)
                idx, x, _ = d.selection()
                assert np.array_equal(idx, np.arange(3 * n))
                r = np.sqrt((fpos[:, 0] * fpos[:, 0] + fpos[:, 1] * fpos[:, 1])
                            + fpos[:, 2] * fpos[:, 2])
                assert same_bits(x, r), (box, lo)
                ref = reference_fields(fpos, vel)
                for f in KINEMATIC_FIELDS:
                    assert same_values(d.kinematic_field(f), ref[f]), (box, lo, f)
                vphi = d.kinematic_field("vphi")[:n]
                assert np.array_equal(np.signbit(vphi), np.signbit(fpos[:n, 0])), (box, lo)
                assert np.signbit(vphi[1]) and vphi[1] == 0.0   # -0.0 stays -0.0
                assert not np.signbit(vphi[0]) and not np.signbit(vphi[2]) and vphi[2] == 0.0
            finally:
                d.close()
    # the fixture's own rows: the reference's bits through the device's wrap
    for bx, box in enumerate(gold["boxes"]):
        box = float(box)
        for s in (0, 5):
            pos = gold[f"pos/{bx}/{s}"]
            for conv, lo in (("center", np.full(3, -0.5 * box)), ("upper", np.zeros(3)),
                             ("minirange", gold[f"lo/{bx}/{s}"])):
                ref = gold[f"ref/{bx}/{s}/{conv}"]
                d = DeviceBins.select(pos, None, frame=Frame(wrap=(box, lo)))
                try:
                    r = np.sqrt((ref[:, 0] * ref[:, 0] + ref[:, 1] * ref[:, 1])
                                + ref[:, 2] * ref[:, 2])
                    assert same_bits(d.selection()[1], r), (box, s, conv)
                finally:
                    d.close()


# ------------------------------------------------------ 3. wrap extents
@pytest.mark.parametrize("n", [1, 63, 1025, SWEEP + 1000])
def test_wrap_extents_bit_identical(gpu, n):
    pos = particles(n)[0]
    for fr in (None, Frame(CENTRE), Frame(CENTRE, VC)):
        got = pdev.wrap_extents(pos, L, frame=fr)
        ref = wrap_extents(pos if fr is None else fr.pos(pos), L)
        assert got.shape == (12,) and same_bits(got, ref), (n, fr, got, ref)
        if fr is not None and n >= 1025:  # a halo at the origin: center on every axis
            assert np.array_equal(choose_lower(got, L), CENTER_LO)
    # arrays resident on the device: the same bits
    dp = nat.DeviceArray.from_host(pos)
    try:
        dev = pdev.wrap_extents(dp.ptr, L, frame=Frame(CENTRE), on_device=True, n=n)
        assert same_bits(dev, wrap_extents(Frame(CENTRE).pos(pos), L))
    finally:
        dp.free()


def test_wrap_extents_nan_empty_and_errors(gpu):
    pos = particles(5000)[0].copy()
    clean = pdev.wrap_extents(pos, L)
    for axis in range(3):
        dirty_pos = pos.copy()
        dirty_pos[1234, axis] = np.nan
        got = pdev.wrap_extents(dirty_pos, L)
        own = slice(4 * axis, 4 * axis + 4)
        assert np.isnan(got[own]).all()
        rest = np.ones(12, dtype=bool)
        rest[own] = False
        assert same_bits(got[rest], clean[rest])
        assert same_values(got, wrap_extents(dirty_pos, L))
        assert choose_lower(got, L)[axis] == 0.0  # a NaN range: upper
    ident = np.tile([np.inf, -np.inf], 6)
    assert same_bits(pdev.wrap_extents(np.zeros((0, 3)), L), ident)
    assert same_bits(pdev.wrap_extents(np.zeros((0, 3)), L, frame=Frame(CENTRE)), ident)
    for bad in (Frame(R=ROT), Frame(CENTRE, R=ROT), Frame(wrap=(L, UPPER_LO)),
                Frame(CENTRE, wrap=(L, CENTER_LO))):
        with pytest.raises(ValueError, match="PBX_FRAME"):
            pdev.wrap_extents(pos, L, frame=bad)
    for bad_L in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="box size"):
            pdev.wrap_extents(pos, bad_L)


# ------------------------------------------------------------ 4. errors
def test_wrap_frame_errors(gpu):
    pos, vel, mass, _ = particles(63)
    good = FRAMES["all"]
    assert good.flags == 23 and good.packed().shape == (19,)
    bad_frames = {}
    for name, (box, lo) in {"L = 0": (0.0, [0.0, 0.0, 0.0]), "L = -1": (-1.0, [0.0, 0.5, 0.0]),
                            "L = inf": (np.inf, [0.0, 0.0, 0.0]), "L = nan": (np.nan, [0.0] * 3),
                            "bad lo": (L, [0.0, 0.25 * L, 0.0]),
                            "lo = +L/2": (L, [0.5 * L, 0.0, 0.0])}.items():
        packed = good.packed()
        packed[15], packed[16:19] = box, lo
        bad_frames[name] = packed
    d = DeviceBins()
    try:
        for name, packed in bad_frames.items():
            for flags in (16, 23):
                with pytest.raises(ValueError, match="PBX_FRAME_WRAP"):
                    nat.call("pbx_profile_set_frame", d._h, flags, nat.dptr(packed))
                with pytest.raises(ValueError, match="PBX_FRAME_WRAP"):
                    kept, out = nat.c_int64(0), np.zeros(18)
                    nat.call("pbx_property_moments_frame", nat.vptr(pos), nat.vptr(vel),
                             nat.vptr(mass), 63, 0, 0, None, None, 0, pdev.MASS, flags,
                             nat.dptr(packed), nat.ctypes.byref(kept), nat.dptr(out))
            # without the flag frame[15..18] is not looked at
            nat.call("pbx_profile_set_frame", d._h, 7, nat.dptr(packed))
        # bit 8 is unassigned: still an error, alone and beside the wrap
        for flags in (8, 8 | 16):
            with pytest.raises(ValueError, match="PBX_FRAME"):
                nat.call("pbx_profile_set_frame", d._h, flags, nat.dptr(good.packed()))
            with pytest.raises(ValueError, match="PBX_FRAME"):
                kept, out = nat.c_int64(0), np.zeros(18)
                nat.call("pbx_property_moments_frame", nat.vptr(pos), nat.vptr(vel), nat.vptr(mass),
                         63, 0, 0, None, None, 0, pdev.MASS, flags, nat.dptr(good.packed()),
                         nat.ctypes.byref(kept), nat.dptr(out))
        # the enclosed pass and the virial radius refuse a bad wrap as well
        for name, packed in bad_frames.items():
            scope = (nat.vptr(pos), nat.vptr(mass), 63, 0, 0, None, None, 0, 16, nat.dptr(packed), 0,
                     None, None, None)
            kept, msum, count = nat.c_int64(0), np.zeros(1), np.zeros(1, dtype=np.int64)
            t = np.ones(1)
            with pytest.raises(ValueError, match="PBX_FRAME_WRAP"):
                nat.call("pbx_property_enclosed", *scope, 1, nat.dptr(t), nat.ctypes.byref(kept),
                         nat.dptr(msum), count.ctypes.data_as(nat.ctypes.POINTER(nat.c_int64)), None)
            radius, it, passes, status = np.zeros(1), nat.c_int64(0), nat.c_int64(0), nat.ctypes.c_int(0)
            with pytest.raises(ValueError, match="PBX_FRAME_WRAP"):
                nat.call("pbx_property_virial_radius", *scope, 1.0, 1e-3, 200, 0, 0.0, 0,
                         nat.dptr(radius), nat.ctypes.byref(it), nat.ctypes.byref(passes),
                         nat.ctypes.byref(kept), nat.ctypes.byref(status))
        # float32 positions with a wrap frame: the existing "frame is set" error
        with pytest.raises(ValueError, match="frame is set"):
            DeviceBins.select(pos.astype(np.float32), mass, into=d, frame=FRAMES["center"])
        # and the frame is usable afterwards
        DeviceBins.select(pos, mass, into=d, frame=FRAMES["center"])
        fpos = FRAMES["center"].pos(pos)
        assert same_bits(d.selection()[1], np.sqrt((fpos[:, 0] * fpos[:, 0] + fpos[:, 1] * fpos[:, 1])
                                                   + fpos[:, 2] * fpos[:, 2]))
    finally:
        d.close()


# -------------------------------------------------------- 5. end to end
BOX = 64.0
GRID = 2.0 ** -20
N_HALO = 20000
UNITS = {"pos": "kpc", "vel": "km s**-1", "mass": "Msol"}


@functools.lru_cache(maxsize=None)
def halo():
    """(broken, whole, centre): a Plummer halo whose offsets are multiples of
    2^-20, placed at a centre on the same grid within 1.0 of a box corner and
    reduced into [0, 64); and the same halo unbroken at the origin.  Every
    operation of the shift and the wrap is exact: the wrapped coordinates are
    the offsets bit for bit."""
    off, _ = plummer(N_HALO, seed=77, rmax=30.0)
    off = np.round(off / GRID) * GRID
    centre = np.round(np.array([BOX - 0.37, 0.61, BOX - 0.83]) / GRID) * GRID
    pos = np.mod(centre + off, BOX)
    rng = np.random.default_rng(78)
    vel = rng.normal(scale=50.0, size=(N_HALO, 3))
    vel[:, 1] += 80.0 * off[:, 0] / np.sqrt(1.0 + off[:, 0] ** 2)  # some rotation about z
    vel[:, 0] -= 80.0 * off[:, 1] / np.sqrt(1.0 + off[:, 1] ** 2)
    mass = rng.uniform(0.5, 1.5, N_HALO)
    fam = {"dm": slice(0, N_HALO // 2), "star": slice(N_HALO // 2, N_HALO)}

    def snap(p):
        return SimSnap({"pos": np.ascontiguousarray(p), "vel": vel.copy(), "mass": mass.copy()},
                       families=fam, units_map=UNITS, properties={"boxsize": BOX})

    assert np.abs(off).max() < 0.5 * BOX
    assert np.array_equal(bits(Frame(centre, wrap=(BOX, np.full(3, -32.0))).pos(pos)), bits(off))
    return snap(pos), snap(off), centre


@pytest.mark.parametrize("convention", ["minirange", "center"])
def test_halo_across_the_box_corner_end_to_end(gpu, convention):
    broken, whole, centre = halo()
    before = np.asarray(broken["pos"]).tobytes()
    scope = Sphere(20.0) & FamilyFilter("star")
    chain = ShiftPosTo(centre).then(WrapBox(convention=convention))
    view = chain(broken)
    assert isinstance(view, FrameView) and view._frame_base is broken
    assert view._frame.flags == (1 | 16)
    assert np.array_equal(view._frame.wrap[1], np.full(3, -32.0))  # center on all three axes
    assert not view._derived  # (the extents came from the device pass, not from a host copy)

    builder = RadialProfileBuilder(ndim=3, weight="mass", bins_type="equaln", nbins=64)
    prof = builder.filter(scope).transform(chain)(broken)
    ref = builder.filter(scope)(whole)
    assert same_bits(np.asarray(prof.bin_edges), np.asarray(ref.bin_edges))
    assert np.array_equal(prof.npart_bins, ref.npart_bins) and prof.npart_bins.sum() > 5000
    assert all(np.array_equal(x, y) for x, y in zip(prof.binind, ref.binind))
    assert same_bits(np.asarray(prof["mass"]["sum"]), np.asarray(ref["mass"]["sum"]))

    re_got = ParamContain("r").filter(scope).transform(chain)(broken)
    re_ref = ParamContain("r").filter(scope)(whole)
    assert same_bits(re_got, re_ref), (re_got, re_ref)
    k_got = KappaRot().filter(scope).transform(chain)(broken)
    k_ref = KappaRot().filter(scope)(whole)
    assert same_bits(k_got, k_ref), (k_got, k_ref)

    # without the wrap the halo is in pieces: every result differs
    shift_only = ShiftPosTo(centre)
    torn = builder.filter(scope).transform(shift_only)(broken)
    assert not np.array_equal(torn.npart_bins, ref.npart_bins)
    assert torn.npart_bins.sum() < ref.npart_bins.sum()
    assert not same_bits(np.asarray(torn.bin_edges), np.asarray(ref.bin_edges))
    assert not same_bits(ParamContain("r").filter(scope).transform(shift_only)(broken), re_ref)
    assert not same_bits(KappaRot().filter(scope).transform(shift_only)(broken), k_ref)
    assert np.asarray(broken["pos"]).tobytes() == before
