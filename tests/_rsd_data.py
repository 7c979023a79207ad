"""Shared by the RadiusAtSurfaceDensity tests and tests/golden/make_golden_rsd.py.

A numpy restatement of the device algorithm (csrc/profile.hip cum_table,
cum_sigma_at, cum_solve_kernel): the reference's statements in Python floats
with every square written as the product ``r * r`` (IEEE: correctly rounded,
what the device computes), where the reference's ``r**2`` on scalars is libm
``pow``.  The restatement also measures how far every decision of the scan
and the bisection stays from its threshold (``Solve.margin_ok``), which is
what lets a test compare the device route with the host route bit for bit.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "radius_at_density.npz"
UNITS = {"pos": "kpc", "vel": "km s**-1", "mass": "Msol"}
NGRID = 256
ITERS = 80
BREAK = 1e-10
ULP = 2.0 ** -52
REL_MARGIN = 1e-9  # the scan's sigma - target, relative to the larger of the two
SAFETY = 16.0      # bisection decisions: this many times sigma's own one-ulp bound


def radii(pos: np.ndarray, r_key: str) -> np.ndarray:
    """r / rxy as the snapshot layer and the selection kernels compute them."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    return np.sqrt((x * x + y * y) + z * z) if r_key == "r" else np.sqrt(x * x + y * y)


def table(r: np.ndarray, m: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(sorted r, cumulative m) in stable order: the device table."""
    order = np.argsort(r, kind="stable")
    return r[order], np.cumsum(m[order])


def sigma_product(r, xs, cum, eps, mode) -> tuple[float, float]:
    """(sigma, bound): _sigma_at_radius with product squares, and the relative
    bound on |sigma - the reference's| when the reference's pow squares differ
    from the products by one ulp: one ulp of each square through the
    subtraction, the multiply by pi and the divide,
    2^-52 (3 + 2 rout^2 / (rout^2 - rin^2)); 3 2^-52 in total mode; 0 where a
    guard returns 0.0 without arithmetic."""
    r, eps = float(r), float(eps)
    if r <= 0:
        return 0.0, 0.0
    if mode == "total":
        hi = int(np.searchsorted(xs, r, side="right"))
        if hi <= 0:
            return 0.0, 0.0
        area = np.pi * (r * r)
        return (0.0, 0.0) if area <= 0 else (float(cum[hi - 1]) / area, 3 * ULP)
    rin = max(r - 0.5 * eps, 0.0)
    rout = r + 0.5 * eps
    if rout <= 0:
        return 0.0, 0.0
    lo = int(np.searchsorted(xs, rin, side="left"))
    hi = int(np.searchsorted(xs, rout, side="right"))
    if hi <= 0 or hi <= lo:
        return 0.0, 0.0
    m_shell = float(cum[hi - 1]) - (float(cum[lo - 1]) if lo > 0 else 0.0)
    a_out, a_in = rout * rout, rin * rin
    area = np.pi * (a_out - a_in)
    if area <= 0:
        return 0.0, 0.0
    return m_shell / area, ULP * (3 + 2 * a_out / (a_out - a_in))


@dataclass
class Solve:
    radius: float
    status: int      # 0 solved, 1 not bracketed
    k: int           # bracket index (-1: none)
    iters: int       # bisection steps run, the one that stopped early included
    broke: int       # 1 if |sigma_mid - target| < 1e-10 stopped the loop
    grid: np.ndarray
    sigma_grid: np.ndarray
    # (what, distance from the threshold, distance required) per decision
    decisions: list = field(default_factory=list)

    @property
    def info(self) -> list[int]:
        return [self.status, self.k, self.iters, self.broke]

    @property
    def margin_ok(self) -> bool:
        return all(d > need for _, d, need in self.decisions)

    def worst(self):
        """The decision closest to its threshold, relative to what it needs."""
        return min(self.decisions, key=lambda t: t[1] / t[2] if t[2] > 0 else np.inf)


def solve_product(xs, cum, eps, mode, target) -> Solve:
    """The device solve (grid, first sign change, 80-step bisection) and the
    margin of each decision it took:

    * the scan: |sigma[j] - target| > 1e-9 max(|sigma[j]|, |target|) at every
      grid point compared (0 .. k+1; all of them without a bracket);
    * the break test: | |sigma_mid - target| - 1e-10 | must exceed 1e-9 of
      the larger of its two terms and 16 times the one-ulp bound of sigma_mid;
    * the bisection product: neither factor sigma - target may be within 16
      times the one-ulp bound of its sigma (then no such ulp flips its sign).

    A margin of 1e-9 relative to sigma cannot be asked of the bisection's own
    differences: a loop that stops at |sigma_mid - target| < 1e-10 with a
    target of order 1 has to pass through differences of 1e-10.  What those
    decisions must survive is the one-ulp perturbation of a squared radius,
    so they are measured against its propagated bound instead."""
    target, eps = float(target), float(eps)
    r_min, r_max = float(xs[0]), float(xs[-1])
    grid = np.linspace(max(r_min, eps), r_max, NGRID)
    sig = np.array([sigma_product(r, xs, cum, eps, mode)[0] for r in grid])
    diff = sig - target
    changes = np.where(np.signbit(diff[:-1]) != np.signbit(diff[1:]))[0]
    k = int(changes[0]) if len(changes) else -1
    out = Solve(np.nan, 1, k, 0, 0, grid, sig)
    last = NGRID - 1 if k < 0 else k + 1
    for j in range(last + 1):
        out.decisions.append((f"grid[{j}]", abs(float(diff[j])),
                              REL_MARGIN * max(abs(float(sig[j])), abs(target))))
    if k < 0:
        return out
    left, right = float(grid[k]), float(grid[k + 1])
    for _ in range(ITERS):
        out.iters += 1
        mid = 0.5 * (left + right)
        s_mid, b_mid = sigma_product(mid, xs, cum, eps, mode)
        d_mid = s_mid - target
        out.decisions.append((f"break[{out.iters}]", abs(abs(d_mid) - BREAK),
                              max(REL_MARGIN * max(abs(d_mid), BREAK), SAFETY * b_mid * abs(s_mid))))
        if abs(d_mid) < BREAK:
            left = right = mid
            out.broke = 1
            break
        s_left, b_left = sigma_product(left, xs, cum, eps, mode)
        d_left = s_left - target
        out.decisions.append((f"left[{out.iters}]", abs(d_left), SAFETY * b_left * abs(s_left)))
        out.decisions.append((f"mid[{out.iters}]", abs(d_mid), SAFETY * b_mid * abs(s_mid)))
        if d_left * d_mid <= 0:
            right = mid
        else:
            left = mid
    out.radius = 0.5 * (left + right)
    out.status = 0
    return out


# ------------------------------------------------------------------ fixture
@dataclass
class Case:
    name: str
    dataset: str
    r_key: str
    mode: str
    eps: float
    mscale: float  # the dataset's masses times this (a power of two)
    target: float
    radius: float  # the reference's (NaN: it raised "Could not bracket ...")
    info: list     # status, bracket index, iterations run, broke


class Fixture:
    """tests/golden/radius_at_density.npz, read once."""

    def __init__(self):
        z = np.load(GOLDEN)
        self.z = z
        self.datasets = [str(s) for s in z["datasets"]]
        self.cases = []
        for c in (str(s) for s in z["cases"]):
            self.cases.append(Case(c, str(z[f"{c}/dataset"]), str(z[f"{c}/r_key"]),
                                   str(z[f"{c}/mode"]), float(z[f"{c}/eps"]),
                                   float(z[f"{c}/mscale"]), float(z[f"{c}/target"]),
                                   float(z[f"{c}/radius"]), [int(v) for v in z[f"{c}/info"]]))

    def pos(self, ds):
        return self.z[f"{ds}/pos"]

    def mass(self, ds, mscale=1.0):
        return self.z[f"{ds}/mass"] * mscale

    def table(self, ds, r_key, mscale=1.0):
        return table(radii(self.pos(ds), r_key), self.mass(ds, mscale))

    def sigma_lists(self):
        """(dataset, r_key, eps, radii, reference sigma total, reference sigma shell)"""
        for ds in self.datasets:
            for r_key in ("r", "rxy"):
                p = f"{ds}/{r_key}"
                yield (ds, r_key, float(self.z[f"{p}/sig_eps"]), self.z[f"{p}/sig_r"],
                       self.z[f"{p}/sigma_total"], self.z[f"{p}/sigma_shell"])


_fixture = None


def fixture() -> Fixture:
    global _fixture
    if _fixture is None:
        _fixture = Fixture()
    return _fixture


def bits(a) -> np.ndarray:
    return np.atleast_1d(np.asarray(a, dtype=np.float64)).view(np.uint64)
