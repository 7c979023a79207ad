"""The inputs of tests/test_gpu_float32.py, pinned on the CPU: each condition
below is a floor without which the GPU test of the same input could not tell
a right float32 kernel from a subtly wrong one.  Only numpy runs here; the
measured share of every condition is printed (pytest -s shows it).
"""
import numpy as np
import pytest

import _f32_data as fd
from _f32_data import F32

N_SMALL = 20_011


def _share(name, hits, total):
    print(f"[float32 inputs] {name}: {hits} of {total} ({100.0 * hits / total:.1f} %)")
    return hits / total


def test_bulk_float32_r_differs_from_rounded_double():
    """float32 arithmetic is not the rounded double evaluation: a kernel that
    computed r2 in double for float32 positions would be visible."""
    pos, m32, m64 = fd.bulk(N_SMALL, 101)
    assert pos.dtype == F32 and m32.dtype == F32 and m64.dtype == np.float64
    assert m64.min() >= 0.5 and m64.max() < 1.5
    for ndim in (3, 2):
        r32 = fd.radius(pos, ndim)
        rd = fd.radius(pos.astype(np.float64), ndim).astype(F32)
        share = _share(f"bulk ndim {ndim}: float32 r != float32(double r)",
                       int((r32 != rd).sum()), len(pos))
        assert share >= 0.10


def test_bulk_fused_multiply_add_differs():
    """x*x + y*y contracted into a fused multiply-add (one rounding: computed
    in double, rounded once) is not the plain float32 evaluation."""
    pos = fd.bulk(N_SMALL, 101)[0]
    x, y = pos[:, 0], pos[:, 1]
    plain = x * x + y * y
    assert plain.dtype == F32
    yy = (y * y).astype(np.float64)  # the product that stays a float32 multiply
    fused = (x.astype(np.float64) * x.astype(np.float64) + yy).astype(F32)
    share = _share("bulk: fma(x, x, y*y) != x*x + y*y", int((plain != fused).sum()), len(pos))
    assert share >= 0.10
    # and it shows in rxy itself, not only in its square
    differ = int((np.sqrt(fused) != np.sqrt(plain)).sum())
    _share("bulk: sqrt of the fused sum != rxy", differ, len(pos))
    assert differ >= 100


@pytest.mark.parametrize("cen", [fd.CEN_EXACT, fd.CEN_INEXACT], ids=["exact", "inexact"])
def test_shell_masks_differ(cen):
    """On the shell the widened-double mask and the float32-evaluated one keep
    different particles, and the sphere keeps about half."""
    pos = fd.shell(cen=cen)
    assert pos.dtype == F32 and pos.shape == (20_000, 3)
    c32 = np.asarray(cen, dtype=np.float64).astype(F32).astype(np.float64)
    assert np.array_equal(c32, cen) == (cen == fd.CEN_EXACT)
    m64 = fd.sphere_mask64(pos, cen, fd.SHELL_R)
    m32 = fd.sphere_mask32(pos, cen, fd.SHELL_R)
    _share(f"shell {cen}: masks differ", int((m64 != m32).sum()), len(pos))
    kept = _share(f"shell {cen}: kept by the double mask", int(m64.sum()), len(pos))
    assert int((m64 != m32).sum()) >= 100
    assert 0.30 <= kept <= 0.70


def _first_rows():
    pos, kind = fd.edge_rows()
    k = len(fd.EDGE_TABLE)
    assert np.array_equal(kind[:k], np.arange(k))
    return pos[:k], dict(zip(fd.EDGE_NAMES, range(k)))


def test_edge_rows_layout():
    pos, kind = fd.edge_rows()
    k = len(fd.EDGE_TABLE)
    assert pos.dtype == F32 and pos.shape[0] >= fd.EDGE_MIN_ROWS and pos.shape[0] > 2 * 4096
    assert np.bincount(kind).min() > 64  # more than one wave per value
    # every repetition holds the same bits
    assert np.array_equal(pos.view(np.uint32), np.tile(pos[:k].view(np.uint32), (len(pos) // k, 1)))
    # the issue's rows are all there
    names = set(fd.EDGE_NAMES)
    assert {"sub_1e-20", "sub_1e-23", "min_normal", "least_sub", "ovf_3e19", "near_ovf", "nan",
            "inf", "neg_zero", "2^24+1", "3_4_5"} <= names


@pytest.mark.parametrize("ndim", [3, 2])
def test_edge_rows_subnormal_and_overflow(ndim):
    p, row = _first_rows()
    tiny = np.finfo(F32).tiny
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        r2 = (x * x + y * y) if ndim == 2 else ((x * x + y * y) + z * z)
    r = fd.radius(p, ndim)
    sub = (r2 > 0) & (r2 < tiny)
    print(f"[float32 inputs] edge rows ndim {ndim}: subnormal non-zero r2 in "
          f"{[fd.EDGE_NAMES[i] for i in np.nonzero(sub)[0]]}")
    assert sub.sum() >= 3
    assert (r[sub] > 0).all()  # flush-to-zero would give 0 here
    # a flushed evaluation (subnormal products and sums replaced by 0) differs
    with np.errstate(all="ignore"):
        sq = [np.where(np.abs(c * c) < tiny, F32(0), c * c) for c in (x, y, z)]
        f2 = sq[0] + sq[1] if ndim == 2 else (sq[0] + sq[1]) + sq[2]
        f2 = np.where(np.abs(f2) < tiny, F32(0), f2)
        rf = np.sqrt(f2)
    assert ((rf != r) & sub).sum() >= 3
    # float32 overflow where double stays finite
    with np.errstate(all="ignore"):
        d = p.astype(np.float64)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + (0 if ndim == 2 else d[:, 2] * d[:, 2])
    ovf = np.isinf(r) & np.isfinite(d2)
    print(f"[float32 inputs] edge rows ndim {ndim}: float32 r infinite, double r2 finite in "
          f"{[fd.EDGE_NAMES[i] for i in np.nonzero(ovf)[0]]}")
    assert ovf.sum() >= 1 and ovf[row["ovf_3e19"]]
    assert np.isfinite(r[row["near_ovf"]])
    # -0.0 gives +0.0; NaN and inf propagate; the exact rows are exact
    assert r[row["neg_zero"]] == 0 and not np.signbit(r[row["neg_zero"]])
    assert np.isnan(r[row["nan"]]) and np.isposinf(r[row["inf"]])
    assert r[row["3_4_5"]] == 5
    assert p[row["2^24+1"], 0] == 2.0 ** 24
    assert r[row["least_sub"]] == 0 and p[row["least_sub"], 0] > 0


def test_edge_rows_origin_sphere_drops_nonfinite():
    """Sphere(1e10) at the origin in double: NaN and inf rows fail the
    comparison (so do the rows beyond 1e10), every other row passes."""
    p, row = _first_rows()
    m = fd.sphere_mask64(p, (0.0, 0.0, 0.0), 1e10)
    assert not m[row["nan"]] and not m[row["inf"]]
    assert not m[row["ovf_3e19"]] and not m[row["near_ovf"]]
    assert m.sum() == len(p) - 4


def test_edge_mass_values():
    m = fd.edge_mass(40)
    assert m.dtype == F32
    tiny = np.finfo(F32).tiny
    assert 0 < m[0] < tiny and m[1] == np.finfo(F32).max
    assert m[2] == 0 and np.signbit(m[2]) and 0 < m[3] < tiny
    assert np.array_equal(m[:5], m[5:10])


def test_family_cases_start_past_zero():
    n = N_SMALL
    cases = fd.family_cases(n)
    assert len(cases) == 4
    for fams in cases:
        assert min(lo for lo, _ in fams) > 0
        assert all(0 < lo < hi <= n for lo, hi in fams)
    assert cases[0][0][0] == 4096 + 1 and cases[0][-1][1] == n - 1
    assert cases[1] == [(1, 2)] and cases[2] == [(n - 1, n)]
    assert cases[3][0][1] == cases[3][1][0] == 4096  # abutting


def test_select_ref_follows_numpy_dtype_rules():
    """The yardstick itself: mask from the widened doubles, x in the
    positions' dtype, masses widened."""
    pos, m32, m64 = fd.bulk(N_SMALL, 101)
    sph = ((0.7, -0.4, 0.2), 5.0)
    fams = fd.family_cases(N_SMALL)[0]
    idx, x, w = fd.select_ref(pos, m32, sph, fams, 3)
    p64 = pos.astype(np.float64)
    d = p64 - np.asarray(sph[0])
    keep = (d * d).sum(axis=1) < 25.0  # (another summation order: compare counts loosely)
    keep &= fd.family_mask(N_SMALL, fams)
    assert abs(int(keep.sum()) - len(idx)) <= 2
    assert idx.dtype == np.int64 and np.all(np.diff(idx) > 0)
    assert np.array_equal(x.astype(F32).astype(np.float64), x)  # float32 values, widened
    assert np.array_equal(w, m32[idx].astype(np.float64))
    _share("bulk: kept by Sphere(5) & families", len(idx), N_SMALL)
    # float64 positions: x in double
    idx2, x2, w2 = fd.select_ref(p64, None, sph, fams, 2)
    assert np.array_equal(idx2, idx) and np.all(w2 == 1.0)
    assert np.array_equal(x2, np.sqrt(p64[idx, 0] * p64[idx, 0] + p64[idx, 1] * p64[idx, 1]))


def test_bits_equal_and_longdouble_sums():
    a = np.array([0.0, -0.0, np.nan, 1.0])
    assert fd.bits_equal(a, a.copy())
    assert not fd.bits_equal(a, np.array([-0.0, -0.0, np.nan, 1.0]))
    assert not fd.bits_equal(a, np.array([0.0, -0.0, 2.0, 1.0]))
    v = np.array([1.0, 2.0, 4.0, 8.0])
    s = fd.longdouble_bin_sums(v, np.array([3, 0, 1]), np.array([0, 1, 1, 3]))
    assert s.dtype == np.longdouble and list(s) == [8.0, 0.0, 3.0]
