"""The float32 snapshot path of the profile selection (pbx_profile_select_typed:
select_onepass<.., float> and the T = float branch of select_xyz in
csrc/profile.hip; DeviceBins.select and RadialProfileBuilder.execute_fused on
the Python side) against numpy itself, at its edges.  The yardstick
(tests/_f32_data.py, select_ref) is numpy's own arithmetic: float32 numpy for
r / rxy (bit for bit), float64 numpy on the widened positions for the Sphere
mask, np.longdouble sums of the widened values for per-bin sums and
oracle/profile_ref.py on the widened x for edges, counts and the CSR.
tests/test_float32_cpu.py pins what the inputs contain.

Which instantiation each test reaches (select_launch: fewer than 1024 tiles
of 4096 in the families' span -> the 1024-thread kernel, else the 256-thread
one):

  test_dtype_matrix        float32 pos: select_onepass<1024, false, float>, 5
                           tiles; float64 pos: <1024, false, double> with the
                           sphere_origin shortcut (origin sphere, ndim 3) and
                           without; load_mass in both widths, mass = NULL
  test_mask_rule           <1024, false, float>, the use_sphere branch of
                           select_xyz<float>
  test_edge_values         <1024, false, float>, 3 tiles; sqrtf and the float32
                           multiplies and adds on subnormal, overflowing and
                           non-finite values; load_mass(float)
  test_span_offsets        select_prep's staged upload at ps / ms = 4 and 8
                           with lo > 0; in_family with one and two ranges
  test_large_span          select_onepass<256, false, float>: 1025 tiles;
                           h2d_staged in 16 MB chunks (50 MB of positions)
  test_device_resident_abi <1024, false, float> on the caller's device
                           pointers (on_device = 1: no staging), lo > 0
  test_user_route          execute_fused -> DeviceBins.select (float32, and
                           the wdev branch with float64 masses), and
                           RadialProfile on a host-filtered float32 view

Counts behind the input conditions (test_float32_cpu.py prints them):
  bulk(20011, 101)   float32 r != float32(double r) on 18.8 % of the rows (ndim
                     2: 16.8 %); fma(x, x, y*y) != x*x + y*y on 16.0 %
  shell, exact       double and float32 masks differ on 475 of 20000 rows,
                     50.0 % kept;  inexact centre: 559 rows, 50.0 % kept
  edge_rows          4 distinct rows with a subnormal non-zero float32 r2
                     (the issue's table alone gives one: (1e-23)^2 rounds to 0
                     and (2^-63)^2 is FLT_MIN itself, so three rows were
                     added); 1 row with r = inf in float32, finite in double

Measured on an MI355X, test_large_span (2.08M kept, 128 equaln bins of about
16,000): worst per-bin error against the longdouble sums, relative, Σw 0 (a
sum of 16,000 float32 values of one binade is exact in double in any order)
and Σx·w 6.6e-16, against the bound 1e-12.  Every other comparison is exact.

Each of these, tried on a copy of csrc/profile.hip, turns the file red:
  the Sphere difference in float32 ((double)(px - (float)cx))   test_mask_rule,
                        all four cases, and nothing else
  no ``#pragma clang fp contract(off)`` in select_xyz            every ndim 3
                        case with float32 positions (27 of 79); the compiler
                        fuses only the + z*z of the 3-D sum, so ndim 2 stays
                        green
  r2 of float32 positions evaluated in double, rounded once      52 of 79: every
                        float32 case of both ndim but test_edge_values[3]
  ``ps = sizeof(double)`` for float32 in select_prep             test_span_offsets
                        (run on the cases [(1, 2)] and [(100, 4096), (4096,
                        8192)], where the wrongly sized host reads stay
                        inside the arrays)
"""
import ctypes
from ctypes import byref, c_int64

import numpy as np
import pytest

from oracle import profile_ref as pr
from pynbodyext import _native as nat
from pynbodyext.filters import FamilyFilter, Sphere
from pynbodyext.profiles import RadialProfile, RadialProfileBuilder
from pynbodyext.profiles._device import PBX_F32, SRC_NONE, SRC_W, SRC_X, DeviceBins
from pynbodyext.simcore import SimSnap

import _f32_data as fd
from _f32_data import F32

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-12  # tests/test_gpu_profile.py: per-bin sums of positive terms

N = 20_011
SEED = 101
SPH_ORIGIN = ((0.0, 0.0, 0.0), 6.0)
SPH_OFF = ((0.7, -0.4, 0.2), 5.0)
SCOPES = {
    "none": (None, None),
    "origin": (SPH_ORIGIN, None),
    "off": (SPH_OFF, None),
    "off_fam": (SPH_OFF, fd.family_cases(N)[0]),
}


def _arrays(pos_dt, mass_dt):
    pos, m32, m64 = fd.bulk(N, SEED)
    p = pos if pos_dt == "f32" else pos.astype(np.float64)
    m = {"f32": m32, "f64": m64, "none": None}[mass_dt]
    return p, m


def check_selection(d, pos, mass, sphere, families, ndim, nbins=128):
    """idx, x, w, minmax, equaln edges, counts and CSR of a selection handle
    against select_ref and the oracle on the widened x."""
    idx_r, x_r, w_r = fd.select_ref(pos, mass, sphere, families, ndim)
    idx, x, w = d.selection(idx=True, x=True, w=True)
    assert d.n == len(idx_r)
    assert np.array_equal(idx, idx_r)
    assert fd.bits_equal(x, x_r)
    assert fd.bits_equal(w, w_r)
    if pos.dtype == F32:  # float32 values, held widened
        assert np.array_equal(x.astype(F32).astype(np.float64), x, equal_nan=True)
    lo, hi = d.minmax()
    assert lo == x_r.min() and hi == x_r.max()
    edges = d.edges_equaln(nbins)
    assert np.array_equal(edges, pr.edges_equaln(x_r, nbins))
    counts = d.assign(edges)
    perm_r, offs_r, counts_r = pr.assign(x_r, edges)
    assert np.array_equal(counts, counts_r)
    perm, offs = d.csr()
    assert np.array_equal(perm, perm_r) and np.array_equal(offs, offs_r)
    return idx_r, x_r, w_r


# ---------------------------------------------------------------- 1 dtypes
@pytest.mark.parametrize("scope", list(SCOPES))
@pytest.mark.parametrize("ndim", [3, 2])
@pytest.mark.parametrize("mass_dt", ["f32", "f64", "none"])
@pytest.mark.parametrize("pos_dt", ["f32", "f64"])
def test_dtype_matrix(gpu, pos_dt, mass_dt, ndim, scope):
    """Every pairing of position and mass dtype (decided independently by
    DeviceBins.select), both x, every scope."""
    pos, mass = _arrays(pos_dt, mass_dt)
    sphere, fams = SCOPES[scope]
    d = DeviceBins.select(pos, mass, sphere=sphere, families=fams, ndim=ndim)
    try:
        assert d._pos_dt == (PBX_F32 if pos_dt == "f32" else 0)
        assert d._mass_dt == (PBX_F32 if mass_dt == "f32" else 0)
        idx, _, _ = check_selection(d, pos, mass, sphere, fams, ndim)
        assert 0.2 * N < len(idx) <= N
    finally:
        d.close()


# ---------------------------------------------------------------- 2 mask
@pytest.mark.parametrize("ndim", [3, 2])
@pytest.mark.parametrize("cen", [fd.CEN_EXACT, fd.CEN_INEXACT], ids=["exact", "inexact"])
def test_mask_rule(gpu, cen, ndim):
    """The Sphere test of float32 positions is evaluated in double on the
    widened coordinates (3-D for either ndim): on the shell that set is not
    the one a float32 subtraction keeps."""
    pos = fd.shell(cen=cen)
    m64 = fd.sphere_mask64(pos, cen, fd.SHELL_R)
    m32 = fd.sphere_mask32(pos, cen, fd.SHELL_R)
    assert int((m64 != m32).sum()) >= 100  # a wrong rule cannot pass
    d = DeviceBins.select(pos, None, sphere=(cen, fd.SHELL_R), ndim=ndim)
    try:
        idx, x, w = d.selection(idx=True, x=True, w=True)
        assert np.array_equal(idx, np.nonzero(m64)[0])
        assert fd.bits_equal(x, fd.radius(pos[m64], ndim).astype(np.float64))
        assert np.all(w == 1.0)
    finally:
        d.close()


# ---------------------------------------------------------------- 3 edges
def _nan_last_equal(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("ndim", [3, 2])
def test_edge_values(gpu, ndim):
    """Subnormal squares, float32 overflow, NaN, inf and -0.0: every row
    kept without a sphere and x bit-equal to numpy's float32 evaluation; an
    origin sphere drops what the double comparison drops; a float32 mass
    column of edge values comes back exactly widened; equaln edges with the
    NaN keys last."""
    pos, kind = fd.edge_rows()
    n = len(pos)
    mass = fd.edge_mass(n)
    x_r = fd.radius(pos, ndim).astype(np.float64)
    row = dict(zip(fd.EDGE_NAMES, range(len(fd.EDGE_NAMES))))
    d = DeviceBins.select(pos, mass, ndim=ndim)
    try:
        idx, x, w = d.selection(idx=True, x=True, w=True)
        assert np.array_equal(idx, np.arange(n))
        assert fd.bits_equal(x, x_r)
        for name in ("sub_1e-20", "sub_3_4", "sub_xyz", "sub_pow2"):  # not flushed
            assert np.all(x[kind == row[name]] > 0), name
        assert np.all(np.isposinf(x[kind == row["ovf_3e19"]]))
        assert not np.signbit(x[kind == row["neg_zero"]]).any()
        assert fd.bits_equal(w, mass.astype(np.float64))
        assert np.signbit(w[2]) and w[2] == 0 and w[0] == float(mass[0]) > 0
        edges = d.edges_equaln(16)
        ref = pr.edges_equaln(x_r, 16)
        assert np.isnan(ref[-1]) and np.isfinite(ref[0])  # np.sort: NaN keys last
        assert _nan_last_equal(edges, ref)
    finally:
        d.close()
    sph = ((0.0, 0.0, 0.0), 1e10)
    keep = fd.sphere_mask64(pos, *sph)
    d = DeviceBins.select(pos, mass, sphere=sph, ndim=ndim)
    try:
        idx, x, w = d.selection(idx=True, x=True, w=True)
        assert np.array_equal(idx, np.nonzero(keep)[0])
        assert not np.isin(kind[idx], [row["nan"], row["inf"]]).any()
        assert len(idx) == n - 4 * (n // len(fd.EDGE_NAMES))
        assert fd.bits_equal(x, x_r[keep]) and np.isfinite(x).all()
        assert fd.bits_equal(w, mass[keep].astype(np.float64))
        assert np.array_equal(d.edges_equaln(16), pr.edges_equaln(x_r[keep], 16))
    finally:
        d.close()


# ---------------------------------------------------------------- 4 offsets
@pytest.mark.parametrize("mass_dt", ["f32", "f64"])
@pytest.mark.parametrize("case", range(4))
def test_span_offsets(gpu, case, mass_dt):
    """Only the families' span is uploaded, at its own byte offset: with NaN
    in every particle outside it, a copy from or to an offset computed with
    the wrong element size shows in x or w."""
    fams = fd.family_cases(N)[case]
    lo, hi = min(a for a, _ in fams), max(b for _, b in fams)
    p, m = _arrays("f32", mass_dt)
    pos, mass = p.copy(), m.copy()
    pos[:lo] = np.nan
    pos[hi:] = np.nan
    mass[:lo] = np.nan
    mass[hi:] = np.nan
    d = DeviceBins.select(pos, mass, families=fams, ndim=3)
    try:
        idx, x, w = d.selection(idx=True, x=True, w=True)
        idx_r, x_r, w_r = fd.select_ref(p, m, None, fams, 3)  # (the clean arrays)
        assert len(idx_r) == sum(b - a for a, b in fams)
        assert np.array_equal(idx, idx_r)
        assert np.isfinite(x).all() and np.isfinite(w).all()
        assert fd.bits_equal(x, x_r) and fd.bits_equal(w, w_r)
        if len(idx_r) > 1:
            check_selection(d, p, m, None, fams, 3, nbins=min(128, len(idx_r)))
    finally:
        d.close()


# ---------------------------------------------------------------- 5 large
def test_large_span(gpu):
    """1025 tiles: the 256-thread float kernel, positions staged in four
    pinned chunks, a span that starts at particle 1000."""
    n = 4_194_304 + 5 + 1000
    fams = [(1000, n)]
    assert -(-(n - 1000) // 4096) == 1025 and 12 * (n - 1000) > 3 * (16 << 20)
    pos, m32, _ = fd.make_bulk(n, 7)
    sph = ((0.7, -0.4, 0.2), 4.6)
    d = DeviceBins.select(pos, m32, sphere=sph, families=fams, ndim=3)
    try:
        idx_r, x_r, w_r = fd.select_ref(pos, m32, sph, fams, 3)
        assert 0.4 * n < len(idx_r) < 0.6 * n
        idx, x, w = d.selection(idx=True, x=True, w=True)
        assert np.array_equal(idx, idx_r)
        assert fd.bits_equal(x, x_r) and fd.bits_equal(w, w_r)
        stats = [(SRC_W, SRC_NONE, 1 << 3), (SRC_X, SRC_W, 0b11)]
        edges, counts, mom = d.binned_equaln(128, None, None, stats)
        assert np.array_equal(edges, pr.edges_equaln(x_r, 128))
        perm_r, offs_r, counts_r = pr.assign(x_r, edges)
        assert np.array_equal(counts, counts_r)
        perm, offs = d.csr()
        assert np.array_equal(perm, perm_r) and np.array_equal(offs, offs_r)
        L = np.longdouble
        sw = fd.longdouble_bin_sums(w_r, perm_r, offs_r)
        sxw = fd.longdouble_bin_sums(x_r.astype(L) * w_r.astype(L), perm_r, offs_r)
        for name, got, ref in (("sum w", mom[0][:, 3], sw), ("sum w (2)", mom[1][:, 0], sw),
                               ("sum x*w", mom[1][:, 1], sxw)):
            err = float(np.max(np.abs(got.astype(L) - ref) / ref))
            print(f"[float32 large span] {name}: worst per-bin relative error {err:.3e}")
            assert err <= SUM_RTOL, name
    finally:
        d.close()


# ---------------------------------------------------------------- 6 C ABI
@pytest.mark.parametrize("ndim", [3, 2])
@pytest.mark.parametrize("scope", ["off_fam", "fam_only"])
def test_device_resident_abi(gpu, scope, ndim):
    """pbx_profile_select_typed with on_device = 1 and PBX_F32 for both
    arrays (the header allows it; DeviceBins.select never does it): float32
    device arrays indexed absolutely, no staging, a span with lo > 0."""
    pos, mass = _arrays("f32", "f32")
    fams = fd.family_cases(N)[0]
    sphere = SPH_OFF if scope == "off_fam" else None
    d_pos, d_mass = nat.DeviceArray.from_host(pos), nat.DeviceArray.from_host(mass)
    assert d_pos.nbytes == 12 * N and d_mass.nbytes == 4 * N
    d = DeviceBins()
    try:
        args, keep = DeviceBins._select_args(d_pos.ptr, d_mass.ptr, sphere, fams, ndim, True, N)
        p_pos, p_mass, n_part, *rest = args
        kept = c_int64(0)
        nat.call("pbx_profile_select_typed", d._h, p_pos, PBX_F32, p_mass, PBX_F32, n_part, *rest,
                 byref(kept))
        del keep
        d.n, d.has_selection = kept.value, True
        check_selection(d, pos, mass, sphere, fams, ndim)
    finally:
        d.close()
        d_pos.free()
        d_mass.free()


# ---------------------------------------------------------------- 7 user route
FAMILIES = {"dm": slice(0, 9000), "star": slice(9000, N)}
NB = 32


def _snapshot(mass_dt):
    pos, mass = _arrays("f32", mass_dt)
    return SimSnap({"pos": pos, "mass": mass}, families=FAMILIES), pos, mass


def _check_profile(prof, pos, mass, bt, ndim):
    key = "r" if ndim == 3 else "rxy"
    fams = [(FAMILIES["star"].start, FAMILIES["star"].stop)]
    idx_r, x_r, w_r = fd.select_ref(pos, mass, SPH_OFF, fams, ndim)
    assert len(prof.sim) == len(idx_r)
    xs = np.asarray(prof.sim[key])
    assert xs.dtype == F32 and np.array_equal(xs, fd.radius(pos[idx_r], ndim))
    edges = pr.EDGE_ALGORITHMS[bt](x_r, NB)  # lin / log: from the float32 min and max
    assert np.array_equal(np.asarray(prof.bin_edges, dtype=np.float64), edges)
    perm_r, offs_r, counts_r = pr.assign(x_r, edges)
    assert np.array_equal(prof.npart_bins, counts_r)
    perm, offs = prof.bins.binind.csr
    assert np.array_equal(perm, perm_r) and np.array_equal(offs, offs_r)
    L = np.longdouble
    sw = fd.longdouble_bin_sums(w_r, perm_r, offs_r)
    sxw = fd.longdouble_bin_sums(x_r.astype(L) * w_r.astype(L), perm_r, offs_r)
    ok = counts_r > 0
    assert ok.sum() >= NB // 2
    msum = np.asarray(prof["mass"]["sum"], dtype=np.float64)
    mean = np.asarray(prof[key], dtype=np.float64)
    assert np.isnan(msum[~ok]).all() and np.isnan(mean[~ok]).all()
    np.testing.assert_allclose(msum[ok], sw[ok].astype(np.float64), rtol=SUM_RTOL)
    np.testing.assert_allclose(mean[ok], (sxw[ok] / sw[ok]).astype(np.float64), rtol=SUM_RTOL)
    med, _ = pr.compute(x_r, w_r, perm_r, offs_r, "median")
    assert np.array_equal(np.asarray(prof[key]["median"], dtype=np.float64), med, equal_nan=True)
    return idx_r


@pytest.mark.parametrize("mass_dt", ["f32", "f64"])
@pytest.mark.parametrize("ndim", [3, 2])
@pytest.mark.parametrize("bt", ["lin", "log", "equaln"])
def test_user_route(gpu, bt, ndim, mass_dt):
    """What a user with a float32 snapshot gets: RadialProfileBuilder behind
    Sphere & FamilyFilter (the fused device selection) and RadialProfile of
    the host-filtered view."""
    sim, pos, mass = _snapshot(mass_dt)
    filt = Sphere(SPH_OFF[1], cen=SPH_OFF[0]) & FamilyFilter("star")
    fused = RadialProfileBuilder(ndim=ndim, weight="mass", bins_type=bt, nbins=NB).filter(filt)(sim)
    idx = _check_profile(fused, pos, mass, bt, ndim)
    sub_mass = np.asarray(fused.sim["mass"])
    assert sub_mass.dtype == mass.dtype and np.array_equal(sub_mass, mass[idx])
    assert np.array_equal(fused.sim.get_index_list(sim), idx)
    plain = RadialProfile(sim[np.asarray(filt(sim))], ndim=ndim, weight="mass", bins_type=bt, nbins=NB)
    _check_profile(plain, pos, mass, bt, ndim)
