"""Pin the multipole content of the Barnes–Hut oracle (oracle/tree_ref.c) to
the long-double Legendre series of tests/_multipole_data.py — CPU only.

The other value tests of the tree compare the device with this oracle, and
tests/test_oracle_tree.py checks the oracle's orders 2-5 only through
properties a wrong coefficient survives.  Here every order of both evaluators,
the root moments and the whole walk (opening decisions included) are compared
with a restatement that shares no arithmetic with them; the conventions are
in _multipole_data's docstring.

Compared: per target |dphi| / |phi| and ||da|| / ||a||; moments scaled by the
node's mass * edge^k as test_gpu_tree.check_structure does.

Measured maxima (the same figures, digit for digit, on two x86-64 hosts):
  full walks, 12 trees x 2 theta x 6 orders x 64 targets   pot 3.0e-15  acc 7.0e-15
  single-node shells, 8 inputs x 6 orders x 120 targets     pot 1.1e-15  acc 9.6e-15
  evaluators called directly on the oracle's own P2M        pot 2.0e-15  acc 1.5e-14
  root moments (through the whole M2M chain)                7.7e-17
  P2M slot by slot                                          4.9e-16
BOUND = 1.2e-13 is 8 x the largest of them (1.47e-14), below the 1e-12 no
bound here may exceed.  Inputs are seeded and the code is deterministic: the
margin covers libm and compiler differences between hosts only.

The shifted cube needs no bound of its own.  Its coordinates are ~2300 edges,
so the float64 centre of mass of a node is off its true place by about
eps * |offset|, and the dipole about the *stored* centre is M * eps * |offset|
instead of M * eps * edge.  The potential evaluators drop the dipole on both
sides, but the oracle's acceleration evaluator of order >= 2 contracts it with
the second derivatives: a term of 2 * eps * |offset| / |d| relative to the
monopole (3.5e-13 on the shells, |offset| / |d| = 2300 and more), which a
series without its k = 1 term misses.  The series here keeps k = 1 in the
acceleration — that is what the evaluator computes — and then agrees on the
shifted cube as on the cube (4.5e-15 against 3.5e-15).

Every opening decision of every reference walk is at least MIN_MARGIN = 1e-9
relative away from equality (measured: 6.6e-5), so no rounding of dist2 can
flip one; the decisions of the oracle are equal per target.

Sensitivity: the five planted errors of ``test_planted_*`` are made in the
series, never in the oracle; each moves the comparison to >= 100 x BOUND for
every order it applies to and, on the single-node shells, to >= 100 x the
fast-mode bound of the device tests (2e-6).
"""
import functools

import numpy as np
import pytest

from oracle import tree as ot

import _multipole_data as md
from _multipole_data import CASES, CASE_IDS, ORDERS, SHELL_CASES, SHELL_THETA, THETAS, L

BOUND = 1.2e-13
FAST = 2e-6      # tests/test_gpu_tree.py, the device's default mode
assert BOUND <= 1e-12
SHELL_IDS = tuple(n for n, _ in SHELL_CASES)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def oracle_walk(name, leaf, theta, order):
    pos, mass = md.inputs(name)
    ref = ot.RefOctree(pos, mass, leaf, order)
    return frozen(*ref.compute_subset(md.self_targets(name), theta))


@functools.lru_cache(maxsize=None)
def oracle_shell(name, order):
    pos, mass = md.inputs(name)
    ref = ot.RefOctree(pos, mass, 8, order)
    pts = md.shell_targets(name).reshape(-1, 3)
    return frozen(ref.potentials_at_points(pts, SHELL_THETA),
                  ref.accelerations_at_points(pts, SHELL_THETA))


def test_moment_order_known_answers():
    """The slot order of the long-double P2M is the oracle's: m[4] = 1/2 sum
    x^2 and m[20] = sum x^4 / 24, and every slot of an asymmetric point set."""
    pos = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    m = md.p2m(pos, np.ones(2), np.zeros(3))
    assert m[0] == 2 and m[1] == 0 and m[4] == 1 and m[20] == L(2) / 24
    assert md.LMN[4] == (2, 0, 0) and md.LMN[20] == (4, 0, 0) and len(set(md.LMN)) == 56
    rng = np.random.default_rng(5)
    pos, mass, c = rng.random((50, 3)), rng.random(50), np.array([0.1, 0.7, -0.2])
    mo = ot.multipole_from_points(pos, mass, c, 5)
    ml = md.p2m(pos, mass, c)
    dev = float(np.max(np.abs(mo - ml) / np.abs(ml)))
    print(f"P2M slots: {dev:.2e}")
    assert dev < BOUND


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_full_walk(case, order):
    """compute_subset against reference_walk at 64 self targets: the accepted
    nodes and leaf particles of every target, potential and acceleration."""
    name, leaf = case
    for theta in THETAS:
        w = md.walk_terms(name, leaf, theta)
        assert w["margin"].min() >= md.MIN_MARGIN
        pot, acc, nn, npp = oracle_walk(name, leaf, theta, order)
        assert np.array_equal(nn, w["nodes"]) and np.array_equal(npp, w["leaf_particles"])
        assert (nn + npp).min() >= 1
        phi, a = md.walk_values(name, leaf, theta, order)
        rp, ra = md.rel_pot(pot, phi), md.rel_acc(acc, a)
        print(f"walk {name} leaf {leaf} theta {theta} order {order}: pot {rp:.2e} acc {ra:.2e} "
              f"margin {w['margin'].min():.1e}")
        assert rp < BOUND and ra < BOUND, (theta, rp, ra)


def test_reference_walk_is_the_cached_walk():
    """reference_walk (one target, from an export) is what walk_terms caches."""
    name, leaf, theta, order = "cube", 8, 0.5, 4
    pos, mass = md.inputs(name)
    export = ot.RefOctree(pos, mass, leaf, order).export()
    phi, acc = md.walk_values(name, leaf, theta, order)
    w = md.walk_terms(name, leaf, theta)
    for slot in (0, 40, 63):
        i = int(md.self_targets(name)[slot])
        p, a, nn, npp, margin = md.reference_walk(export, order, theta, pos[i], i, pos, mass)
        assert p == phi[slot] and np.array_equal(a, acc[slot])
        assert (nn, npp, margin) == (w["nodes"][slot], w["leaf_particles"][slot], w["margin"][slot])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", SHELL_IDS)
def test_single_node_shells(name, order):
    """at_points at 1, 1.5 and 3 root edges, theta 1.5: the root alone is
    accepted, so the value is one node's series about the root's centre."""
    pt, at, walks = md.shell_terms(name)
    assert np.all(walks[:, 0] == 1) and np.all(walks[:, 1] == 0)
    assert walks[:, 2].min() >= md.MIN_MARGIN
    pot, acc = oracle_shell(name, order)
    phi, a = md.combine(pt, at, order)
    rp, ra = md.rel_pot(pot, phi), md.rel_acc(acc, a)
    top = float(np.max(np.abs(pt[:, md.eo_of(order)] / phi)))
    print(f"shell {name} order {order}: pot {rp:.2e} acc {ra:.2e} (top term {top:.1e} of phi)")
    assert rp < BOUND and ra < BOUND, (rp, ra)


@pytest.mark.parametrize("name", SHELL_IDS)
def test_evaluators_directly(name):
    """gravity_potential_multipole / gravity_accel_multipole on the oracle's
    own P2M and derivative tensors, every order, against node_series."""
    pos, mass = md.inputs(name)
    com = md.ref_tree(name, 8)[1]["com"][0]
    mom = ot.multipole_from_points(pos, mass, com, 5)
    pt, at, _ = md.shell_terms(name)
    pts = md.shell_targets(name).reshape(-1, 3)
    worst = [0.0, 0.0]
    for order in ORDERS:
        pot, acc = np.zeros(len(pts)), np.zeros((len(pts), 3))
        for j, t in enumerate(pts):
            dx, dy, dz = com - t
            D = ot.potential_derivatives(dx, dy, dz, 0.0, max(order, 1))
            pot[j] = ot.gravity_potential_multipole(mom, D, order)
            acc[j] = ot.gravity_accel_multipole(mom, D, order)
        phi, a = md.combine(pt, at, order)
        rp, ra = md.rel_pot(pot, phi), md.rel_acc(acc, a)
        worst = [max(worst[0], rp), max(worst[1], ra)]
        assert rp < BOUND and ra < BOUND, (order, rp, ra)
    print(f"evaluators {name}: pot {worst[0]:.2e} acc {worst[1]:.2e}")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_root_moments(case):
    """The root's 56 moments (P2M in the leaves, M2M up the whole chain)
    against the long-double P2M of all particles about the root's centre."""
    name, leaf = case
    pos, mass = md.inputs(name)
    e = ot.RefOctree(pos, mass, leaf, 5).export()
    ml = md.p2m(pos, mass, e["com"][0])
    scale = L(e["mass"][0]) * L(2 * e["half"][0]) ** md.DEG
    dev = float(np.max(np.abs(e["mom"][0] - ml) / scale))
    big = float(np.max(np.abs(ml[4:]) / scale[4:]))
    print(f"root moments {name} leaf {leaf}: {dev:.2e} (largest moment {big:.1e} of the scale)")
    assert dev < BOUND
    if name in ("rod_x", "rod_y", "rod_z"):  # one family of components, the rest exactly 0
        axis = "xyz".index(name[-1])
        off = np.array([sum(t) != t[axis] for t in md.LMN])
        assert np.all(e["mom"][0][off] == 0) and np.all(ml[off] == 0)
        assert np.all(np.abs(ml[~off][2:]) > 0)


# ------------------------------------------------------------ sensitivity
def planted_deviation(order, walk_kw=None, **planted):
    """(largest oracle-vs-mutant deviation over all full walks and shells,
    largest over the shells alone) with the error planted in the series,
    relative to the oracle's value."""
    swap = bool((walk_kw or {}).get("swap_yz"))
    every, shells = 0.0, 0.0
    for name, leaf in CASES:
        for theta in THETAS:
            pot, acc, _, _ = oracle_walk(name, leaf, theta, order)
            phi, a = md.walk_values(name, leaf, theta, order, swap_yz=swap, **planted)
            every = max(every, md.rel_pot(phi, pot.astype(L)), md.rel_acc(a, acc.astype(L)))
    for name in SHELL_IDS:
        pt, at, _ = md.shell_terms(name, swap_yz=swap)
        pot, acc = oracle_shell(name, order)
        phi, a = md.combine(pt, at, order, **planted)
        shells = max(shells, md.rel_pot(phi, pot.astype(L)), md.rel_acc(a, acc.astype(L)))
    return max(every, shells), shells


PLANTED = {
    "1-drop-top-potential-term": (ORDERS, None, dict(drop_top=True)),
    "2-scale-top-potential-term": (ORDERS, None, dict(scale_top=1.001)),
    "3-acceleration-through-eo": ((2, 3, 4, 5), None, dict(acc_through_eo=True)),
    "4-swap-y-z": ((2, 3, 4, 5), dict(swap_yz=True), {}),
}


@pytest.mark.parametrize("which", list(PLANTED))
def test_planted_error_is_seen(which):
    """Each error planted in the series moves the comparison with the oracle
    to >= 100 x BOUND, and on the single-node shells to >= 100 x FAST, on at
    least one input, for every order it applies to (3 and 4 change nothing
    below order 2: eo = 0 there)."""
    orders, walk_kw, planted = PLANTED[which]
    for order in orders:
        every, shells = planted_deviation(order, walk_kw, **planted)
        print(f"planted {which} order {order}: {every:.2e} (shells {shells:.2e})")
        assert every >= 100 * BOUND, (order, every)
        assert shells >= 100 * FAST, (order, shells)


def test_planted_opening_test_with_equality():
    """Planted error 5: <= instead of < in the opening test.  Sixteen unit
    masses at (+-1, +-1, +-1) and (+-1/2, +-1/2, +-1/2) and a massless target
    at (4, 0, 0): the root has size2 = 25 and its centre of mass is exactly
    the origin, so at theta = 1.25 (theta^2 = 1.5625) the target sits on
    size2 == theta^2 * dist2 = 1.5625 * 16 with every value exact in binary.
    The oracle opens the root (strict <); the mutant accepts it."""
    g = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    pos = np.concatenate([g, 0.5 * g, [[4.0, 0.0, 0.0]]])
    mass = np.concatenate([np.ones(16), [0.0]])
    theta = 1.25
    for order in ORDERS:
        ref = ot.RefOctree(pos, mass, 8, order)
        e = ref.export()
        assert e["size2"][0] == 25.0 and np.all(e["com"][0] == 0.0) and e["leaf_off"][0] < 0
        assert theta * theta * 16.0 == 25.0
        pot, acc, nn, npp = ref.compute_subset(np.array([16]), theta)
        p, a, n_nodes, n_leaf, margin = md.reference_walk(e, order, theta, pos[16], 16, pos, mass)
        assert margin == 0.0
        assert (n_nodes, n_leaf) == (int(nn[0]), int(npp[0])) == (0, 16)
        assert md.rel_pot(pot, p[None]) < BOUND and md.rel_acc(acc, a[None]) < BOUND
        p, a, n_nodes, n_leaf, _ = md.reference_walk(e, order, theta, pos[16], 16, pos, mass,
                                                     accept_equal=True)
        assert (n_nodes, n_leaf) == (1, 0)
        dev = max(md.rel_pot(pot, p[None]), md.rel_acc(acc, a[None]))
        print(f"planted 5 order {order}: counts (1, 0) against (0, 16), values {dev:.2e}")
        assert dev >= 100 * BOUND
