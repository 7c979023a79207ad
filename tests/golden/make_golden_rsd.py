#!/usr/bin/env python3
"""Generate the RadiusAtSurfaceDensity fixture from the REFERENCE's own code.

Run here only (needs /root/reference; never on the GPU box, not collected by
pytest):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rsd.py

It loads /root/reference/pynbodyext/properties/base.py by file path.  The
names that module imports are provided as minimal stand-ins:
pynbody.array.SimArray (an ndarray view with ``units`` / ``sim``),
pynbodyext.calculate (``Param`` and a ``PropertyBase`` with ``.dataclass`` and
an ``_in_sim_units`` that passes numbers through) and the
pynbodyext.filters.filt names.  RadiusAtSurfaceDensity.calculate and
_sigma_at_radius then run on plain numpy arrays.  Nothing from the reference
is copied into the repository: tests/golden/radius_at_density.npz holds the
input arrays (at most a few thousand rows), the parameters of each case and
the reference's outputs — radii, sigma at listed radii and, per case, the
bracket index, the number of bisection steps and whether the 1e-10 break
fired (read off the reference's own calls of _sigma_at_radius) — with the
numpy version used.

The script is the gatekeeper of the margin (tests/_rsd_data.py,
solve_product): a case enters the fixture only if the solve restated with
product squares takes every decision outside its margin AND returns the
reference's bits, bracket index, step count and break flag.  A case that
cannot meet that is an error here, never a skipped test.
"""
from __future__ import annotations

import dataclasses
import importlib.util
import sys
import types
import typing
from pathlib import Path

import numpy as np

REF = Path("/root/reference/pynbodyext/properties/base.py")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))

import _rsd_data as rd  # noqa: E402  (tests/_rsd_data.py: the product-square restatement)


# ---------------------------------------------------------------- stand-ins
class _Unit:
    def __truediv__(self, other):
        return _Unit()

    def __pow__(self, p):
        return _Unit()


class SimArray(np.ndarray):
    def __new__(cls, data):
        return np.asarray(data).view(cls)

    def __array_finalize__(self, obj):
        self.units = getattr(obj, "units", None)
        self.sim = getattr(obj, "sim", None)

    def in_units(self, unit, **kw):
        return self


class Param:
    def __init__(self, default=dataclasses.MISSING, *, field_name=None):
        self.default = default

    def __class_getitem__(cls, item):
        return cls


class PropertyBase:
    def __class_getitem__(cls, item):
        return cls

    @classmethod
    def dataclass(cls, target):
        for name, v in list(vars(target).items()):
            if isinstance(v, Param):
                if v.default is dataclasses.MISSING:
                    delattr(target, name)
                else:
                    setattr(target, name, v.default)
        return dataclasses.dataclass(target, eq=False)

    def _in_sim_units(self, value, sim_parameter, sim, target_units=None):
        assert isinstance(value, (int, float))  # (the cases give numbers)
        return float(value)


class Params:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __getitem__(self, key):
        return self.__dict__[key]


class Sim:
    """pos / mass / r / rxy as SimArray views; its own ancestor."""

    def __init__(self, pos, mass):
        self.arrays = {"pos": pos, "mass": mass, "r": rd.radii(pos, "r"),
                       "rxy": rd.radii(pos, "rxy")}

    def __getitem__(self, key):
        a = SimArray(self.arrays[key])
        a.units = _Unit()
        return a

    @property
    def ancestor(self):
        return self


def load_reference():
    pyn = types.ModuleType("pynbody")
    arr = types.ModuleType("pynbody.array")
    arr.SimArray = SimArray
    pyn.array = arr
    ext = types.ModuleType("pynbodyext")
    ext.__path__ = []
    calc = types.ModuleType("pynbodyext.calculate")
    calc.Param, calc.PropertyBase = Param, PropertyBase
    filters = types.ModuleType("pynbodyext.filters")
    filters.__path__ = []
    filt = types.ModuleType("pynbodyext.filters.filt")
    filt.Annulus = filt.BandPass = type("Filter", (), {})
    filt.ValueLike = typing.Any
    props = types.ModuleType("pynbodyext.properties")
    props.__path__ = []
    sys.modules.update({"pynbody": pyn, "pynbody.array": arr, "pynbodyext": ext,
                        "pynbodyext.calculate": calc, "pynbodyext.filters": filters,
                        "pynbodyext.filters.filt": filt, "pynbodyext.properties": props})
    spec = importlib.util.spec_from_file_location("pynbodyext.properties.base", REF)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.RadiusAtSurfaceDensity


# ---------------------------------------------------------------- inputs
def directions(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def ds_plummer():
    """3000 particles of a Plummer sphere cut at r = 12, total mass about 100."""
    rng = np.random.default_rng(7101)
    n = 3000
    r = np.minimum((rng.random(n) ** (-2.0 / 3.0) - 1.0) ** -0.5, 12.0 * rng.random(n) ** 0.25)
    return directions(rng, n) * r[:, None], rng.uniform(0.5, 1.5, n) * (100.0 / n)


def _light(rng, n):
    r = rng.uniform(0.5, 9.5, n)
    return directions(rng, n) * r[:, None], np.full(n, 2.0 ** -10)


def ds_jump():
    """59 light particles and one heavy one inside them: sigma(<r) steps
    across any target of order 1 at the heavy particle's radius."""
    rng = np.random.default_rng(7102)
    pos, mass = _light(rng, 60)
    pos[17] = directions(rng, 1)[0] * 4.2
    mass[17] = 128.0
    return pos, mass


def ds_edge():
    """The heavy particle is the outermost one: the bracket is the last grid interval."""
    rng = np.random.default_rng(7103)
    pos, mass = _light(rng, 60)
    pos[41] = np.array([6.0, -7.5, 2.5])
    mass[41] = 512.0
    return pos, mass


def ds_dyadic():
    """1500 equal masses on the x axis at radii k/64 (ties; none at 300..302 /
    64): radii, their squares, r +- eps/2 with eps = 1/32 and the cumulative
    mass are all exact."""
    rng = np.random.default_rng(7104)
    n = 1500
    allowed = np.array([k for k in range(1, 769) if k not in (300, 301, 302)])
    k = rng.choice(allowed, n)
    pos = np.zeros((n, 3))
    pos[:, 0] = rng.choice([-1.0, 1.0], n) * (k / 64.0)
    return pos, np.full(n, 2.0 ** -4)


DATASETS = {"plummer": ds_plummer, "jump": ds_jump, "edge": ds_edge, "dyadic": ds_dyadic}
SIG_EPS = {"plummer": 0.5, "jump": 0.01, "edge": 0.01, "dyadic": 2.0 ** -5}

# name, dataset, r_key, mode, eps, mscale, target
CASES = [
    ("plummer_total_r", "plummer", "r", "total", 0.01, 1.0, 1.0),
    ("plummer_total_rxy", "plummer", "rxy", "total", 0.01, 1.0, 1.25),
    ("plummer_shell_r", "plummer", "r", "shell", 0.5, 1.0, 1.0),
    ("plummer_shell_rxy", "plummer", "rxy", "shell", 0.5, 1.0, 0.75),
    ("plummer_first_interval", "plummer", "rxy", "total", 0.01, None, None),  # (chosen below)
    ("plummer_no_bracket", "plummer", "r", "total", 0.01, 1.0, -1.0),
    ("jump_total_rxy", "jump", "rxy", "total", 0.01, 1.0, 1.0),
    ("jump_total_r", "jump", "r", "total", 0.01, 1.0, 1.5),
    ("jump_shell_r", "jump", "r", "shell", 0.1, 2.0 ** -5, 1.0),
    ("edge_last_interval", "edge", "r", "total", 0.01, 1.0, 1.0),
    ("dyadic_total_r", "dyadic", "r", "total", 2.0 ** -5, 1.0, 1.0),
    ("dyadic_shell_rxy", "dyadic", "rxy", "shell", 2.0 ** -5, 1.0, 0.5),
]


def first_interval_target(xs, cum):
    """(mscale, target): a power of two and a two-digit target between
    sigma(grid[0]) and sigma(grid[1]) of the scaled masses."""
    probe = rd.solve_product(xs, cum, 0.01, "total", 0.0)
    t0 = 0.5 * (probe.sigma_grid[0] + probe.sigma_grid[1])
    mscale = 2.0 ** -round(np.log2(t0))
    return mscale, round(t0 * mscale, 2)


def sigma_radii(xs, eps):
    """r <= 0, shells clamped at 0, radii equal to a particle's and half a
    shell away from one (the searchsorted sides), between and beyond."""
    j = [0, 1, len(xs) // 3, len(xs) // 2, len(xs) - 2, len(xs) - 1]
    pick = xs[j]
    return np.concatenate([[0.0, -0.0, -1.0, 0.25 * eps, 0.5 * eps, 0.75 * eps], pick,
                           pick - 0.5 * eps, pick + 0.5 * eps, 0.5 * (xs[j[2]] + xs[j[2] + 1:][:1]),
                           [301.0 / 64.0, 0.5 * xs[0], 2.0 * xs[-1]]])


def reference_run(cls, sim, r_key, mode, eps, target):
    """(radius or NaN, [status, k, iterations, broke]) of the reference's
    calculate, the last three read off its calls of _sigma_at_radius: 256 for
    the grid, then two per bisection step, one in the step that breaks."""
    calls = []
    plain = cls.__dict__["_sigma_at_radius"].__func__

    def counted(r_val, r_sorted, m_cum, e, m):
        s = plain(r_val, r_sorted, m_cum, e, m)
        calls.append(s)
        return s

    cls._sigma_at_radius = staticmethod(counted)
    try:
        prop = cls(target=target, parameter="mass", mode=mode, r_key=r_key, eps=eps)
        params = Params(target=target, parameter="mass", mode=mode, r_key=r_key, eps=eps)
        try:
            radius = float(prop.calculate(sim, params))
            status = 0
        except ValueError as e:
            assert str(e) == "Could not bracket target surface density", e
            radius, status = np.nan, 1
    finally:
        cls._sigma_at_radius = staticmethod(plain)
    assert len(calls) >= rd.NGRID
    diff = np.array(calls[:rd.NGRID], dtype=float) - target
    changes = np.where(np.signbit(diff[:-1]) != np.signbit(diff[1:]))[0]
    extra = len(calls) - rd.NGRID
    if status:
        assert extra == 0 and len(changes) == 0
        return radius, [1, -1, 0, 0]
    broke = extra % 2
    return radius, [0, int(changes[0]), (extra + 1) // 2, broke]


def main():
    cls = load_reference()
    out = {"numpy_version": np.array(np.__version__), "datasets": np.array(list(DATASETS))}
    data = {}
    for ds, make in DATASETS.items():
        pos, mass = make()
        assert len(pos) <= 4096
        data[ds] = (pos, mass)
        out[f"{ds}/pos"], out[f"{ds}/mass"] = pos, mass
        for r_key in ("r", "rxy"):
            r = rd.radii(pos, r_key)
            idx = np.argsort(r)  # (the reference's own order)
            r_sorted, m_cum = r[idx], np.cumsum(mass[idx])
            xs, cum = rd.table(r, mass)
            # ties carry equal dyadic masses: their order does not show
            assert np.array_equal(r_sorted, xs) and np.array_equal(m_cum, cum), (ds, r_key)
            eps = SIG_EPS[ds]
            rr = sigma_radii(xs, eps)
            p = f"{ds}/{r_key}"
            out[f"{p}/sig_eps"], out[f"{p}/sig_r"] = np.array(eps), rr
            for mode in ("total", "shell"):
                ref = np.array([cls._sigma_at_radius(x, r_sorted, m_cum, eps, mode) for x in rr])
                out[f"{p}/sigma_{mode}"] = ref
                for x, s in zip(rr, ref):  # the bound the GPU test asserts holds here already
                    got, b = rd.sigma_product(x, xs, cum, eps, mode)
                    assert abs(got - s) <= b * abs(s), (ds, r_key, mode, x, got, s)

    seen = set()
    names = []
    for name, ds, r_key, mode, eps, mscale, target in CASES:
        pos, mass = data[ds]
        if target is None:
            mscale, target = first_interval_target(*rd.table(rd.radii(pos, r_key), mass))
        m = mass * mscale
        xs, cum = rd.table(rd.radii(pos, r_key), m)
        radius, info = reference_run(cls, Sim(pos, m), r_key, mode, eps, target)
        mine = rd.solve_product(xs, cum, eps, mode, target)
        what, dist, need = mine.worst()
        print(f"{name:24s} target={target:<6g} mscale={mscale:<10g} radius={radius!r:24} info={info} "
              f"worst margin {what}: {dist:.3e} (needs > {need:.3e})")
        # the gate: every decision outside its margin, the reference's bits and path
        assert mine.margin_ok, (name, what, dist, need)
        assert mine.info == info, (name, mine.info, info)
        assert np.array_equal(rd.bits(mine.radius), rd.bits(radius)), (name, mine.radius, radius)
        assert 0.1 <= abs(target) <= 10.0, name  # order 1 in the snapshot's units
        if info[0] == 0 and not info[3]:  # no break: the root sits on a jump of sigma
            assert info[2] == rd.ITERS
        names.append(name)
        for key, val in (("dataset", ds), ("r_key", r_key), ("mode", mode), ("eps", eps),
                         ("mscale", mscale), ("target", target), ("radius", radius),
                         ("info", np.array(info, dtype=np.int64))):
            out[f"{name}/{key}"] = np.array(val)
        seen.add(mode)
        seen.add(r_key)
        if info[0]:
            seen.add("no bracket")
        else:
            seen.add("break" if info[3] else "full")
            seen.add(f"k={info[1]}") if info[1] in (0, rd.NGRID - 2) else None
            if not info[3] and np.any(xs == radius):
                seen.add("onto a particle")
    need = {"total", "shell", "r", "rxy", "no bracket", "break", "full", "k=0", f"k={rd.NGRID - 2}",
            "onto a particle"}
    assert need <= seen, need - seen
    out["cases"] = np.array(names)
    np.savez_compressed(OUT / "radius_at_density.npz", **out)
    size = (OUT / "radius_at_density.npz").stat().st_size
    print(f"wrote radius_at_density.npz: {len(names)} cases, {size} bytes")


if __name__ == "__main__":
    main()
