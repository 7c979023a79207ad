"""Inputs and the numpy yardstick of the float32 selection tests
(tests/test_float32_cpu.py on the CPU, tests/test_gpu_float32.py on the GPU).
No tests in here.

``bulk``          well-scaled float32 positions with masses in both dtypes;
``shell``         particles within +-8 float32 ulps of a sphere's surface, so
                  that a mask evaluated in float32 keeps other particles than
                  one evaluated on the widened doubles;
``edge_rows``     float32 edge values: subnormal squares, squares that
                  overflow float32 but not double, NaN, inf, -0.0;
``family_cases``  family range lists that start past particle 0;
``select_ref``    the selection restated in numpy: the mask in float64 on the
                  widened positions, r / rxy in the positions' own dtype (numpy
                  evaluates ``x * x + y * y`` as separate, unfused float32
                  operations and a correctly rounded sqrt), masses widened.

Every builder is cached and returns read-only arrays: copy before changing.
"""
import functools

import numpy as np

F32 = np.float32

CEN_EXACT = (0.5, -0.25, 0.125)  # exactly representable in float32
CEN_INEXACT = (0.1, -0.2, 0.3)   # not representable
SHELL_R = 10.0


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def make_bulk(n, seed):
    """(pos float32 (n,3), mass float32, mass float64), uncached."""
    rng = np.random.default_rng(seed)
    pos = rng.normal(scale=3.0, size=(n, 3)).astype(F32)
    m64 = rng.uniform(0.5, 1.5, n)
    return _freeze(pos, m64.astype(F32), m64)


bulk = functools.lru_cache(maxsize=None)(make_bulk)


@functools.lru_cache(maxsize=None)
def shell(n=20_000, cen=CEN_EXACT, R=SHELL_R, seed=41):
    """(pos float32 (n,3),): unit directions times R * (1 + k * 2**-24), k
    uniform in -8..8, plus ``cen``, rounded to float32."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    k = rng.integers(-8, 9, n)
    rad = R * (1.0 + k * 2.0 ** -24)
    pos = (d * rad[:, None] + np.asarray(cen, dtype=np.float64)).astype(F32)
    return _freeze(pos)[0]


def sphere_mask64(pos, cen, R):
    """The Sphere test in float64 on the widened positions (pbx.h)."""
    p = np.asarray(pos).astype(np.float64)
    c = np.asarray(cen, dtype=np.float64)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
        return ((dx * dx + dy * dy) + dz * dz) < float(R) * float(R)


def sphere_mask32(pos, cen, R):
    """The WRONG rule a float32 kernel could apply: centre rounded to
    float32, float32 subtraction and float32 squares."""
    p = np.asarray(pos, dtype=F32)
    c = np.asarray(cen, dtype=np.float64).astype(F32)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
        s = (dx * dx + dy * dy) + dz * dz
        assert s.dtype == F32
        return s.astype(np.float64) < float(R) * float(R)


def radius(pos, ndim):
    """r (ndim 3) or rxy (ndim 2) in the dtype of ``pos``: numpy's own
    arithmetic, the semantics of sim["r"] / sim["rxy"]."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    with np.errstate(all="ignore"):
        r2 = (x * x + y * y) if ndim == 2 else ((x * x + y * y) + z * z)
        r = np.sqrt(r2)
    assert r.dtype == pos.dtype
    return r


# the distinct rows of edge_rows(), by name
EDGE_TABLE = (
    ("sub_1e-20", (1e-20, 0.0, 0.0)),          # r2 = 1e-40: subnormal
    ("sub_1e-23", (1e-23, 1e-23, 0.0)),        # squares below half the least subnormal: 0
    ("min_normal", (2.0 ** -63, 2.0 ** -63, 0.0)),  # squares = FLT_MIN, r2 = 2**-125
    ("least_sub", (1e-45, 0.0, 0.0)),          # a subnormal coordinate, r2 = 0
    # (the four rows above give one subnormal non-zero r2; three more, so
    # that a flushing multiply, a flushing add and a sqrtf without denormal
    # scaling each meet several)
    ("sub_3_4", (3e-21, 4e-21, 0.0)),          # r2 = 2.5e-41
    ("sub_xyz", (1e-22, 2e-21, 5e-21)),        # x*x = 1e-44: seven least subnormals
    ("sub_pow2", (2.0 ** -70, 2.0 ** -68, 0.0)),   # r2 = 17 * 2**-140, exact
    ("ovf_3e19", (3e19, 0.0, 0.0)),            # 9e38 > FLT_MAX: r = inf, finite in double
    ("near_ovf", (1e19, 1e19, 1e19)),          # 3e38 < FLT_MAX: finite
    ("nan", (np.nan, 1.0, 1.0)),
    ("inf", (np.inf, 0.0, 0.0)),
    ("neg_zero", (-0.0, -0.0, -0.0)),
    ("2^24+1", (16777217.0, 1.0, 0.0)),        # rounds to 2**24 on the way in
    ("3_4_5", (3.0, 4.0, 0.0)),
)
EDGE_NAMES = tuple(n for n, _ in EDGE_TABLE)
EDGE_MIN_ROWS = 8200  # three tiles of 4096, more than one wave of 64 per value


@functools.lru_cache(maxsize=None)
def edge_rows():
    """(pos float32 (n,3), kind int64 (n,)): EDGE_TABLE repeated in order to
    at least EDGE_MIN_ROWS rows; kind[i] indexes EDGE_TABLE / EDGE_NAMES."""
    k = len(EDGE_TABLE)
    reps = -(-EDGE_MIN_ROWS // k)
    with np.errstate(all="ignore"):
        table = np.array([row for _, row in EDGE_TABLE], dtype=np.float64).astype(F32)
    pos = np.ascontiguousarray(np.tile(table, (reps, 1)))
    kind = np.tile(np.arange(k, dtype=np.int64), reps)
    return _freeze(pos, kind)


# a float32 mass column of edge values: a subnormal, FLT_MAX, -0.0, the
# least subnormal and an ordinary value
EDGE_MASS = (1e-40, float(np.finfo(F32).max), -0.0, 1e-45, 1.25)


@functools.lru_cache(maxsize=None)
def edge_mass(n):
    m = np.resize(np.array(EDGE_MASS, dtype=np.float64).astype(F32), n)
    return _freeze(m)[0]


def family_cases(n):
    """Family range lists whose span starts past particle 0."""
    return (
        [(4097, 9000), (12000, n - 1)],  # one past a tile boundary, a gap, one short of n
        [(1, 2)],
        [(n - 1, n)],
        [(100, 4096), (4096, 8192)],     # abutting at a tile boundary
    )


def family_mask(n, families):
    m = np.zeros(n, dtype=bool)
    for lo, hi in families:
        m[lo:hi] = True
    return m


def select_ref(pos, mass, sphere, families, ndim):
    """(idx int64, x float64, w float64) of pbx_profile_select_typed in
    numpy: the Sphere test (3-D for either ndim) in float64 on the widened
    positions; x = r / rxy in the dtype of ``pos``, widened; w = the kept
    masses widened, or ones."""
    n = len(pos)
    keep = np.ones(n, dtype=bool)
    if sphere is not None:
        keep &= sphere_mask64(pos, sphere[0], sphere[1])
    if families is not None:
        keep &= family_mask(n, families)
    idx = np.nonzero(keep)[0].astype(np.int64)
    x = radius(pos[idx], ndim).astype(np.float64)
    w = np.ones(len(idx)) if mass is None else mass[idx].astype(np.float64)
    return idx, x, w


def bits_equal(a, b):
    """Same float64 bit patterns (so +0.0 != -0.0), any NaN equal to any NaN."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and
                np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def longdouble_bin_sums(values, perm, offsets):
    """Per-bin sums of ``values[perm]`` over the CSR in np.longdouble,
    returned as longdouble (empty bins 0)."""
    v = np.asarray(values)[perm].astype(np.longdouble)
    nb = len(offsets) - 1
    out = np.zeros(nb, dtype=np.longdouble)
    for b in range(nb):
        out[b] = v[offsets[b]:offsets[b + 1]].sum(dtype=np.longdouble)
    return out
