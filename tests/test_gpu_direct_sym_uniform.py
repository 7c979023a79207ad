"""The two instantiations of the symmetric direct sum (csrc/direct_sym.hip):
the uniform-mass pair loop (all masses bitwise equal: the mass is applied
once per flushed partial sum) and the general one, each checked against the
oracle at symmetric-path sizes, with pbx_direct_sym_path_stats telling which
of them ran.

Sizes: 8192 = the smallest symmetric size (3 superblocks of 3072, 1024 pads);
9217 = 3 x 3072 + 1 (3071 pads, the last real particle alone in a superblock).
Tolerances are test_gpu_direct.py's: 1e-6 in fast mode (raw v_rsq_f64), 1e-10
in precise mode; potentials per particle, accelerations by vector norm.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import gravity as og
from pynbodyext import _engine
from pynbodyext import _native as nat
from pynbodyext.parallel import ShardedDirect
from pynbodyext.synthetic import plummer

pytestmark = pytest.mark.gpu

TIGHT = 1e-10
SYM_FAST = 1e-6
CROSS = 1e-12  # general against uniform kernel, precise mode, masses one ulp apart
SIZES = [8192, 9217]
POT, ACC = nat.WANT_POT, nat.WANT_ACC


def rel_pot(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def rel_acc(a, b):
    return float(np.max(np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)))


def path_stats():
    u, g = ctypes.c_int64(), ctypes.c_int64()
    nat.call("pbx_direct_sym_path_stats", ctypes.byref(u), ctypes.byref(g))
    return u.value, g.value


@functools.lru_cache(maxsize=None)
def positions(n):
    pos, _ = plummer(n, seed=700 + n)
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def masses(n, kind):
    if kind == "uniform":
        m = np.full(n, 1.0 / n)
    else:
        m = np.random.default_rng(n).uniform(0.5, 1.5, n) / n
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def reference(n, kind):
    """Oracle potentials and accelerations (kind None: masses=None)."""
    pos = positions(n)
    if kind is None:
        ref = og.direct_potentials(pos), og.direct_accelerations(pos)
    else:
        m = masses(n, kind)
        ref = og.direct_potentials(pos, m), og.direct_accelerations(pos, m)
    for a in ref:
        a.setflags(write=False)
    return ref


def solve(pos, mass, want, precise):
    """The bench / multi-GPU path on one rank -> (pot, acc, uniform launches,
    general launches of this solve); a quantity not wanted is None."""
    u0, g0 = path_stats()
    with nat.precise_mode(precise):
        s = ShardedDirect(None, len(pos), pos, mass)
        s.gather_sources()
        s.solve(want)
        pot, acc = s.results()
    u1, g1 = path_stats()
    return (pot if want & POT else None, acc if want & ACC else None, u1 - u0, g1 - g0)


def check(pot, acc, n, kind, precise):
    ref_p, ref_a = reference(n, kind)
    lim = TIGHT if precise else SYM_FAST
    rp = rel_pot(pot, ref_p) if pot is not None else 0.0
    ra = rel_acc(acc, ref_a) if acc is not None else 0.0
    print(f"n={n} masses={kind} precise={precise}: pot_rel={rp:.3e} acc_rel={ra:.3e} (< {lim:g})")
    assert rp < lim and ra < lim, (rp, ra)


@pytest.mark.parametrize("want", [POT, ACC, POT | ACC])
@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_uniform_mass(gpu, n, precise, want):
    pot, acc, du, dg = solve(positions(n), masses(n, "uniform"), want, precise)
    assert (du, dg) == (1, 0)
    check(pot, acc, n, "uniform", precise)


def test_masses_none_runs_uniform(gpu):
    """masses=None (unit masses) through the host entry points."""
    n = 8192
    pos = positions(n)
    u0, g0 = path_stats()
    pot = _engine.direct_potentials_py(pos)
    acc = _engine.direct_accelerations_py(pos)
    u1, g1 = path_stats()
    assert (u1 - u0, g1 - g0) == (2, 0)
    check(pot, acc, n, None, False)


@pytest.mark.parametrize("want", [POT, ACC, POT | ACC])
@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_random_masses_general(gpu, n, precise, want):
    """Unequal masses at symmetric sizes: which mass multiplies which side of
    a pair is checked by the oracle."""
    pot, acc, du, dg = solve(positions(n), masses(n, "random"), want, precise)
    assert (du, dg) == (0, 1)
    check(pot, acc, n, "random", precise)


@functools.lru_cache(maxsize=None)
def uniform_precise(n):
    pot, acc, du, dg = solve(positions(n), masses(n, "uniform"), POT | ACC, True)
    assert (du, dg) == (1, 0)
    return pot, acc


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("n", SIZES)
def test_one_ulp_off_takes_general_path(gpu, n, where):
    """One mass one ulp away from the rest: the general kernel runs, and in
    precise mode it agrees with the uniform kernel on the equal masses."""
    i = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    m = masses(n, "uniform").copy()
    m[i] = np.nextafter(m[i], 1.0)
    pot, acc, du, dg = solve(positions(n), m, POT | ACC, True)
    assert (du, dg) == (0, 1)
    upot, uacc = uniform_precise(n)
    rp, ra = rel_pot(pot, upot), rel_acc(acc, uacc)
    print(f"n={n} ulp at {i}: general vs uniform pot_rel={rp:.3e} acc_rel={ra:.3e} (< {CROSS:g})")
    assert rp < CROSS and ra < CROSS, (rp, ra)


def test_bench_path_uniform(gpu):
    """What bench.py times: ShardedDirect on one rank with equal masses."""
    n = 8192
    pos, mass = positions(n), masses(n, "uniform")
    u0, g0 = path_stats()
    s = ShardedDirect(None, n, pos, mass)
    s.gather_sources()
    s.solve()
    pot, acc = s.results()
    u1, g1 = path_stats()
    assert (u1 - u0, g1 - g0) == (1, 0)
    check(pot, acc, n, "uniform", bool(nat.get_precise()))
