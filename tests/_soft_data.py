"""Inputs and an independent yardstick for the softened-gravity tests
(tests/test_oracle_softened.py on the CPU, tests/test_gpu_softened.py on the
GPU).  No tests in here.

``soft_h``            per-particle softenings spanning two decades, with rows
                      of 0, negative and NaN softenings at fixed indices;
``direct_longdouble`` the softened direct sums of the reference
                      (crates/gravity/src/direct.rs:370-658 with the kernels
                      of kernel.rs:41-128) restated as whole-array numpy in
                      ``np.longdouble``: another summation order, another
                      precision and no shared code with oracle/gravity_ref.c.
"""
import functools

import numpy as np

R2_TINY = np.finfo(np.float64).tiny  # f64::MIN_POSITIVE, direct.rs:7

ZERO_ROWS = slice(0, None, 97)
NEG_ROWS = slice(5, None, 101)
NAN_ROWS = slice(7, None, 103)


@functools.lru_cache(maxsize=None)
def soft_h(n, seed, median=0.02, sigma=1.2):
    """median * exp(N(0, sigma)), rows [::97] = 0, [5::101] = -0.01,
    [7::103] = NaN.  Read-only and cached: copy before changing it."""
    h = median * np.exp(np.random.default_rng(seed).normal(0.0, sigma, n))
    h[ZERO_ROWS] = 0.0
    h[NEG_ROWS] = -0.01
    h[NAN_ROWS] = np.nan
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def tree_inputs():
    """(pos, mass, h) of the softened tree tests: at leaf 8, theta 0.5 the
    h_max guard rejects thousands of nodes the unsoftened walk accepts
    (pinned by test_oracle_softened.py::test_guard_fires)."""
    from pynbodyext.synthetic import plummer

    pos, mass = plummer(6000, seed=11)
    for a in (pos, mass):
        a.setflags(write=False)
    return pos, mass, soft_h(6000, 12)


DIRECT_SIZES = (300, 600, 4097, 8192, 9000)


@functools.lru_cache(maxsize=None)
def direct_inputs(n):
    """(pos, mass, h) of the softened direct-sum tests: softenings of the
    order of the interparticle distance, so that all three branches of the
    spline are taken (test_oracle_softened.py::test_spline_branches_populated)."""
    from pynbodyext.synthetic import plummer

    pos, mass = plummer(n, seed=900 + n)
    for a in (pos, mass):
        a.setflags(write=False)
    # (300 particles have few close pairs: a larger median keeps the innermost
    # spline branch populated there too)
    return pos, mass, soft_h(n, 950 + n, median=0.3 if n < 600 else 0.15, sigma=1.0)


@functools.lru_cache(maxsize=None)
def edge_inputs(single_nan=False):
    """(pos, mass, h, targets) at n = 300 with every softening edge value:
      rows 0, 97, ...     h = 0;  rows 5, 106, 207  h < 0;  rows 7, 110, 213  NaN
                          (``single_nan``: only row 7 — Rust's f64::max gives
                          NaN only for a pair of two NaNs, so a lone NaN row
                          must stay finite in the all-particles form);
      rows 5, 6           close neighbours, both negative (Plummer squares h);
      rows 20, 21         coincident, h = 0.05 on one and 0 on the other: the
                          pair is softened with 0.05, finite;
      rows 30, 31         coincident, h = 0 on both: Newtonian, 0 * inf;
      row 40              h = 0.05, alone.
    targets: 70 points; the first four are the positions of rows 40 (finite),
    30 (two sources of h = 0), 5 (negative: max(h_j, 0) = 0) and 7 (NaN -> 0)."""
    from pynbodyext.synthetic import plummer

    pos, mass = plummer(300, seed=77)
    h = soft_h(300, 78, median=0.3, sigma=1.0).copy()
    if single_nan:
        h[110] = h[213] = 0.02
    h[6] = -0.02
    pos[6] = pos[5] + np.array([0.004, -0.003, 0.002])
    pos[21] = pos[20]
    h[20], h[21] = 0.05, 0.0
    pos[31] = pos[30]
    h[30] = h[31] = 0.0
    h[40] = 0.05
    tgt = plummer(70, seed=79)[0] * 1.2
    tgt[:4] = pos[[40, 30, 5, 7]]
    for a in (pos, mass, h, tgt):
        a.setflags(write=False)
    return pos, mass, h, tgt


def spline_branch_counts(pos, h, max_rows=None, rows=1024):
    """Unordered pairs (i < j) by spline branch (u < 0.5, 0.5 <= u < 1, u >= 1
    or Newtonian) in the all-particles form, u = r / fmax(h_i, h_j); with
    ``max_rows`` only the pairs whose i is below it (a lower bound)."""
    n = len(pos)
    inner = mid = outer = 0
    stop = n if max_rows is None else min(n, max_rows)
    for a in range(0, stop, rows):
        b = min(a + rows, stop)
        d = pos[None, :, :] - pos[a:b, None, :]
        r = np.sqrt((d * d).sum(axis=2) + R2_TINY)
        hp = np.fmax(h[a:b, None], h[None, :])
        with np.errstate(all="ignore"):
            u = np.where(hp > 0, r / hp, np.inf)
        upper = np.arange(n)[None, :] > np.arange(a, b)[:, None]
        inner += int(((u < 0.5) & upper).sum())
        mid += int(((u >= 0.5) & (u < 1.0) & upper).sum())
        outer += int((~(u < 1.0) & upper).sum())
    return inner, mid, outer


def _w2(u):
    """Springel W2(u) (kernel.rs:85-106); NaN falls through to -1/u."""
    u2 = u * u
    u3 = u2 * u
    u4 = u2 * u2
    u5 = u4 * u
    L = u.dtype.type
    inner = L(16) / 3 * u2 - L(48) / 5 * u4 + L(32) / 5 * u5 - L(14) / 5
    mid = 1 / (15 * u) + L(32) / 3 * u2 - 16 * u3 + L(48) / 5 * u4 - L(32) / 15 * u5 - L(16) / 5
    return np.where(u < 0.5, inner, np.where(u < 1.0, mid, -1 / u))


def _w2_prime(u):
    """dW2/du (kernel.rs:108-128)."""
    u2 = u * u
    u3 = u2 * u
    u4 = u2 * u2
    L = u.dtype.type
    inner = L(32) / 3 * u - L(192) / 5 * u3 + 32 * u4
    mid = -1 / (15 * u2) + L(64) / 3 * u - 48 * u2 + L(192) / 5 * u3 - L(32) / 3 * u4
    return np.where(u < 0.5, inner, np.where(u < 1.0, mid, 1 / u2))


def direct_longdouble(pos, mass, h, kernel, targets=None):
    """(potentials, accelerations) of the softened direct sum, float64 values
    of an ``np.longdouble`` evaluation.

    ``targets`` None: the all-particles form — softening fmax(h_i, h_j) (Rust's
    f64::max: NaN only when both are), the self pair left out.  Otherwise the
    sum at ``targets`` over all sources with softening fmax(h_j, 0).
    ``kernel`` 0 Plummer, 1 cubic spline; ``h`` None means no softening.
    r = sqrt(r^2 + f64::MIN_POSITIVE) as in direct.rs.  O(n * m) memory: for
    n <= 600.
    """
    L = np.longdouble
    p = np.asarray(pos, dtype=L)
    m = np.asarray(mass, dtype=L)
    hh = np.zeros(len(p), dtype=L) if h is None else np.asarray(h, dtype=L)
    self_form = targets is None
    t = p if self_form else np.asarray(targets, dtype=L)
    d = p[None, :, :] - t[:, None, :]  # source - target
    r2 = (d * d).sum(axis=2) + L(R2_TINY)
    r = np.sqrt(r2)
    hp = np.fmax(hh[:, None], hh[None, :]) if self_form else np.fmax(hh, L(0))[None, :]
    hp = np.broadcast_to(hp, r.shape)
    with np.errstate(all="ignore"):
        if kernel == 0:
            s2 = r2 + hp * hp
            phi = -1 / np.sqrt(s2)
            g = 1 / (np.sqrt(s2) * s2)
        else:
            newton = hp <= 0
            hs = np.where(newton, L(1), hp)
            u = r / hs
            phi = np.where(newton, -1 / r, _w2(u) / hs)
            g = np.where(newton, 1 / (r2 * r), _w2_prime(u) / (hs * hs) / r)
    if self_form:
        k = np.arange(len(p))
        phi[k, k] = 0
        g[k, k] = 0
    pot = (phi * m[None, :]).sum(axis=1)
    acc = ((g * m[None, :])[:, :, None] * d).sum(axis=1)
    return pot.astype(np.float64), acc.astype(np.float64)
