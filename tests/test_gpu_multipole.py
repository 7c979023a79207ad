"""The device tree (csrc/tree.hip: binomial P2M, xor-butterfly M2M, detraced
order-2/3 evaluators) against the long-double Legendre series of
tests/_multipole_data.py, which shares no arithmetic with it nor with the
oracle it was written to agree with.  tests/test_oracle_multipole.py pins the
oracle to the same series on the CPU and shows that the series, with a
wrong term planted, is >= 1e-4 away.

  full walk    compute_potentials / compute_accelerations at 64 self targets
               per tree against reference_walk on the oracle's tree (links,
               leaf lists and float64 centres of mass are bit-equal on both
               sides, test_gpu_tree.check_structure), orders 0-5, theta 0.5
               and 0.9; info()'s accepted-node and leaf-pair totals equal the
               oracle's sums over all targets;
  single node  potentials_at_points / accelerations_at_points at 1, 1.5 and 3
               root edges with theta 1.5 against node_series of all particles
               about the root's centre.  info() covers at_points: 120 nodes,
               0 leaf pairs.  Only here is a wrong top-order term visible in
               fast mode: in a theta 0.5 walk it is diluted far below 2e-6;
               on rod_d the top term of every order is >= 0.29 of phi;
  moments      export_moments of every internal node of the rods and of the
               two-scale input against the long-double P2M of the node's
               particles, scaled by mass * edge^k.

Bounds are the project's own (tests/test_gpu_tree.py), not tightened from the
measurements.  Maxima measured on an MI355X (potential / acceleration):
                          full walk            single node
  precise  TIGHT 1e-9     2.8e-15 / 1.8e-12    3.9e-15 / 3.5e-13
  fast     FAST  2e-6     8.5e-8  / 6.9e-7     1.5e-7  / 5.4e-7
  moments        1e-12    2.6e-16 of mass * edge^k (rods and two-scale, 52-94
                          internal nodes each, orders 2-5)
Every tree made the oracle's opening decisions in both modes.  The precise
acceleration is within 3e-14 at orders 0, 1, 4 and 5.  At orders 2 and 3 it
is 1.8e-12 on the shifted cube (3.5e-13 on its shells) and 6e-13 on the rods:
the detraced order-2/3 evaluators carry no dipole ("zero about the COM"),
the general ones and the oracle contract the rounding residue
M * eps * |com| of the dipole about the stored centre of mass with the second
derivatives, 2 * eps * |com| / |d| of the monopole
(test_oracle_multipole.py) — 500 times below TIGHT at |com| = 2300 edges.
The largest fast figures are rod_d's (its top terms are of the size of the
monopole); cube, Plummer, shifted and two-scale stay below 2.7e-8 / 1.4e-7.
"""
import functools

import numpy as np
import pytest

from oracle import tree as ot
from pynbodyext import _engine
from pynbodyext import _native as nat

import _multipole_data as md
from _multipole_data import CASES, CASE_IDS, ORDERS, SHELL_CASES, SHELL_THETA, THETAS, L

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
FAST = 2e-6
MOMENTS = 1e-12
SHELL_IDS = tuple(n for n, _ in SHELL_CASES)
MODES = [pytest.param(False, id="precise"), pytest.param(True, id="fast", marks=pytest.mark.fast)]


@pytest.fixture(autouse=True)
def _precise(request):
    """Precise walk unless the parameter set is marked ``fast``."""
    with nat.precise_mode("fast" not in request.keywords):
        yield


@functools.lru_cache(maxsize=None)
def oracle_totals(name, leaf, theta, order):
    """(accepted nodes, leaf pairs) of the oracle summed over all targets."""
    pos, mass = md.inputs(name)
    _, _, nn, npp = ot.RefOctree(pos, mass, leaf, order).compute_subset(np.arange(len(pos)), theta, 1)
    return int(nn.sum()), int(npp.sum())


@pytest.mark.parametrize("fast", MODES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_full_walk(gpu, case, order, fast):
    name, leaf = case
    assert nat.get_precise() == (not fast)
    pos, mass = md.inputs(name)
    idx = md.self_targets(name)
    dev = _engine.Octree(pos, mass, leaf, order)
    for theta in THETAS:
        pot = dev.compute_potentials(theta)
        cnt_p = dev.info()
        acc = dev.compute_accelerations(theta)
        cnt_a = dev.info()
        totals = oracle_totals(name, leaf, theta, order)
        assert (cnt_p["node_interactions"], cnt_p["leaf_pairs"]) == totals
        assert (cnt_a["node_interactions"], cnt_a["leaf_pairs"]) == totals
        phi, a = md.walk_values(name, leaf, theta, order)
        rp, ra = md.rel_pot(pot[idx], phi), md.rel_acc(acc[idx], a)
        print(f"walk {'fast' if fast else 'precise'} {name} leaf {leaf} theta {theta} "
              f"order {order}: pot {rp:.2e} acc {ra:.2e}")
        bound = FAST if fast else TIGHT
        assert rp < bound and ra < bound, (theta, rp, ra)
    dev.close()


@pytest.mark.parametrize("fast", MODES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", SHELL_IDS)
def test_single_node(gpu, name, order, fast):
    assert nat.get_precise() == (not fast)
    pos, mass = md.inputs(name)
    pts = np.ascontiguousarray(md.shell_targets(name).reshape(-1, 3))
    pt, at, walks = md.shell_terms(name)
    assert np.all(walks[:, 0] == 1) and np.all(walks[:, 1] == 0)
    dev = _engine.Octree(pos, mass, 8, order)
    pot = dev.potentials_at_points(pts, SHELL_THETA)
    cnt_p = dev.info()
    acc = dev.accelerations_at_points(pts, SHELL_THETA)
    cnt_a = dev.info()
    for cnt in (cnt_p, cnt_a):
        assert (cnt["node_interactions"], cnt["leaf_pairs"]) == (len(pts), 0)
    phi, a = md.combine(pt, at, order)
    rp, ra = md.rel_pot(pot, phi), md.rel_acc(acc, a)
    print(f"shell {'fast' if fast else 'precise'} {name} order {order}: pot {rp:.2e} acc {ra:.2e}")
    bound = FAST if fast else TIGHT
    assert rp < bound and ra < bound, (rp, ra)
    dev.close()


@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("case", [c for c in CASES if c[0].startswith("rod_") or c[0] == "two_scale"],
                         ids=[i for i in CASE_IDS if i.startswith(("rod_", "two_scale"))])
def test_moments(gpu, case, order):
    name, leaf = case
    pos, mass = md.inputs(name)
    dev = _engine.Octree(pos, mass, leaf, order)
    d = dev.export()
    first = d["links"][:, 0]
    tree = dict(first=first, next=d["links"][:, 1], perm=d["perm"],
                leaf_off=np.where(first == -1, d["leaf"][:, 0], -1), leaf_len=d["leaf"][:, 1])
    nc = md.NCOEF[order]
    mom = dev.export_moments(nc)
    internal = np.flatnonzero(first != -1)
    assert len(internal) >= 30
    worst, seen = 0.0, 0
    for k in internal:
        ids = md.node_particles(tree, k)
        seen += len(ids) if k == 0 else 0
        m_node = d["com"][k, 3]
        assert m_node > 0
        ml = md.p2m(pos[ids], mass[ids], d["com"][k, :3])[:nc]
        scale = L(m_node) * L(2 * d["center"][k, 3]) ** md.DEG[:nc]
        worst = max(worst, float(np.max(np.abs(mom[k] - ml) / scale)))
    assert seen == len(pos)
    print(f"moments {name} leaf {leaf} order {order}: {worst:.2e} over {len(internal)} nodes")
    assert worst < MOMENTS
    dev.close()
