"""Softened gravity (KernelKind.Plummer / Spline, per-particle h) on every
walk and direct-sum path, against the oracle (oracle/tree_ref.c,
oracle/gravity_ref.c) and, for the direct sum, against the long-double
restatement of tests/_soft_data.py.  tests/test_oracle_softened.py pins, on
the CPU, that these inputs make the softened code decide differently from
the unsoftened code: the h_max guard rejects thousands of nodes, all three
spline branches are populated, the edge rows mean what is said here.

Inputs: ``soft_h`` softenings span three decades and hold rows of 0, of
-0.01 and of NaN.  In the tree every softening passes through max(h, 0)
(tree.rs), so those rows are unsoftened; in the all-particles direct sum the
pair softening is the plain hi.max(hj) (direct.rs:395,472): a negative pair
stays negative (Plummer squares it, the spline treats it as Newtonian) and a
pair of two NaNs is NaN.  Rows whose reference value is NaN must be NaN on
the device and the others finite (``check_direct``).

Bounds (the project's own, tests/test_gpu_tree.py / test_gpu_direct.py) and
the maxima measured on an MI355X over each case group (potential /
acceleration):
  contract              1e-5
  tree precise  TIGHT   1e-9    1.4e-15 / 9.9e-15
  tree fast     FAST    2e-6    3.8e-8  / 1.3e-7
  direct        DIRECT  1e-10   1.2e-14 / 1.1e-14  (Newton-refined in both modes)
  long double           1e-10   2.3e-15 / 2.5e-15  (the oracle is within 1e-12 of it)
Every target of every tree case made the oracle's opening decisions.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import gravity as og
from oracle import tree as ot
from pynbodyext import _engine
from pynbodyext import _native as nat
from pynbodyext.gravity import Gravity, KernelKind
from pynbodyext.synthetic import plummer

from _soft_data import direct_inputs, direct_longdouble, edge_inputs, soft_h, tree_inputs
from test_gpu_tree import check_structure

pytestmark = pytest.mark.gpu

TOL = 1e-5
TIGHT = 1e-9
FAST = 2e-6
DIRECT = 1e-10
THETA = 0.5
LEAF = 8
POT, ACC = nat.WANT_POT, nat.WANT_ACC


@pytest.fixture(autouse=True)
def _precise(request):
    """Precise walk unless the test (or the parameter set) is marked ``fast``."""
    with nat.precise_mode("fast" not in request.keywords):
        yield


def rel_pot(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b))) if len(b) else 0.0


def rel_acc(a, b):
    if not len(b):
        return 0.0
    return float(np.max(np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)))


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------- tree
@functools.lru_cache(maxsize=None)
def tree_ref(order, kernel, softened=True):
    """(RefOctree, pot, acc, accepted nodes, leaf pairs per target) of the
    tree inputs; ``kernel`` None with ``softened`` False: the unsoftened tree."""
    pos, mass, h = tree_inputs()
    ref = ot.RefOctree(pos, mass, LEAF, order, softenings=h if softened else None, kernel=kernel)
    return (ref,) + frozen(*ref.compute_subset(np.arange(len(pos)), THETA))


@functools.lru_cache(maxsize=None)
def unsoftened_totals():
    _, _, _, nn, npairs = tree_ref(0, None, False)
    return int(nn.sum()), int(npairs.sum())


def check_values(label, pot_d, acc_d, pot_r, acc_r, bound):
    rp, ra = rel_pot(pot_d, pot_r), rel_acc(acc_d, acc_r)
    print(f"{label}: pot {rp:.2e} acc {ra:.2e}")
    assert np.isfinite(pot_d).all() and np.isfinite(acc_d).all()
    assert rp < TOL and ra < TOL
    assert rp < bound and ra < bound, (rp, ra)


def walk_and_check(label, dev, pot_r, acc_r, nn_r, np_r, theta, bound):
    """check_walk of test_gpu_tree.py with the reference given (decision
    totals equal, values at the contract and at ``bound``), printing the
    maxima; returns (pot, acc, (accepted nodes, leaf pairs))."""
    pot_d = dev.compute_potentials(theta)
    cnt = dev.info()
    acc_d = dev.compute_accelerations(theta)
    totals = (cnt["node_interactions"], cnt["leaf_pairs"])
    assert totals == (int(nn_r.sum()), int(np_r.sum()))
    check_values(label, pot_d, acc_d, pot_r, acc_r, bound)
    return pot_d, acc_d, totals


def leaf_order(dev, n):
    d_idx = nat.DeviceArray(8 * n)
    dev._leaf_particles_device(0, n, None, None, d_idx.ptr)
    order = d_idx.download(np.empty(n, dtype=np.int64))
    d_idx.free()
    assert np.array_equal(np.sort(order), np.arange(n))
    return order


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("order", [0, 1, 2, 3, 4, 5])
def test_tree_orders_precise(gpu, order, kernel):
    """(a) every softened precise instantiation: structure (h_max bit for bit
    with 0, negative and NaN softenings inside the nodes), decisions, values."""
    pos, mass, h = tree_inputs()
    ref, pot_r, acc_r, nn_r, np_r = tree_ref(order, kernel)
    dev = _engine.Octree(pos, mass, LEAF, order, h, kernel)
    assert dev.export()["hmax"] is not None and ref.export()["hmax"] is not None
    check_structure(dev, ref, order)
    _, _, totals = walk_and_check(f"precise order {order} kernel {kernel}", dev, pot_r, acc_r, nn_r,
                                  np_r, THETA, TIGHT)
    nn0, np0 = unsoftened_totals()
    assert totals[0] <= nn0 - 1000 and totals[1] > np0  # the guard fired
    dev.close()


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("order", [0, 3, 5])
def test_tree_per_target_decisions(gpu, order, kernel):
    """(b) every target's accepted nodes + leaf pairs equal the oracle's (the
    totals alone could hide compensating errors); the totals differ from an
    unsoftened device tree's."""
    pos, mass, h = tree_inputs()
    n = len(pos)
    _, _, _, nn_r, np_r = tree_ref(order, kernel)
    dev = _engine.Octree(pos, mass, LEAF, order, h, kernel)
    d_pot, d_cost = nat.DeviceArray(8 * n), nat.DeviceArray(4 * n)
    dev._compute_range_device(THETA, POT, 0, n, 1, d_pot.ptr, None, d_cost.ptr)
    soft_info = dev.info()
    cost = d_cost.download(np.empty(n, dtype=np.int32)).astype(np.int64)
    order_idx = leaf_order(dev, n)
    want = (nn_r + np_r)[order_idx]
    bad = np.flatnonzero(cost != want)
    print(f"order {order} kernel {kernel}: {len(bad)} of {n} targets decide differently")
    assert len(bad) == 0, (bad[:10], cost[bad[:10]], want[bad[:10]])
    plain = _engine.Octree(pos, mass, LEAF, order)
    plain.compute_potentials(THETA)
    plain_info = plain.info()
    assert (plain_info["node_interactions"], plain_info["leaf_pairs"]) == unsoftened_totals()
    assert soft_info["node_interactions"] <= plain_info["node_interactions"] - 1000
    assert soft_info["leaf_pairs"] > plain_info["leaf_pairs"]
    for a in (d_pot, d_cost):
        a.free()
    dev.close()
    plain.close()


@pytest.mark.fast
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("order", [0, 2, 3, 5])
def test_tree_fast_mode(gpu, order, kernel):
    """(c) the fast (raw v_rsq_f64) softened walks: the oracle's decisions,
    values within FAST."""
    pos, mass, h = tree_inputs()
    _, pot_r, acc_r, nn_r, np_r = tree_ref(order, kernel)
    dev = _engine.Octree(pos, mass, LEAF, order, h, kernel)
    walk_and_check(f"fast order {order} kernel {kernel}", dev, pot_r, acc_r, nn_r, np_r, THETA, FAST)
    dev.close()


@pytest.mark.parametrize("fast", [pytest.param(False, id="precise"),
                                  pytest.param(True, id="rawrsq", marks=pytest.mark.fast)])
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("order", [1, 3, 5])
def test_tree_pot_and_acc_in_one_walk(gpu, order, kernel, fast):
    """(d) the WANT_POT | WANT_ACC instantiation (the sharded walk) on two
    ranges that start inside a wave: the oracle at the mode's bound and, for
    orders <= 3 (explicit FMA accumulation), bit-equal to the separate walks."""
    assert nat.get_precise() == (not fast)
    pos, mass, h = tree_inputs()
    n = len(pos)
    _, pot_r, acc_r, _, _ = tree_ref(order, kernel)
    dev = _engine.Octree(pos, mass, LEAF, order, h, kernel)
    pot_full, acc_full = dev.compute_potentials(THETA), dev.compute_accelerations(THETA)
    order_idx = leaf_order(dev, n)
    d_pot, d_acc = nat.DeviceArray(8 * n), nat.DeviceArray(24 * n)
    for first, count in ((37, 1990), (2027, 3973)):
        assert first % 64 and first + count <= n
        dev._compute_range_device(THETA, POT | ACC, first, count, 1, d_pot.ptr, d_acc.ptr, None)
        p = d_pot.download(np.empty(count))
        a = d_acc.download(np.empty((count, 3)))
        ids = order_idx[first:first + count]
        check_values(f"pot+acc order {order} kernel {kernel} fast {fast} [{first}, +{count})", p, a,
                     pot_r[ids], acc_r[ids], FAST if fast else TIGHT)
        if order <= 3:
            assert np.array_equal(p, pot_full[ids]) and np.array_equal(a, acc_full[ids])
    for a in (d_pot, d_acc):
        a.free()
    dev.close()


@pytest.mark.parametrize("order,kernel,fast", [
    (1, 0, False), (1, 1, False), (3, 0, False), (3, 1, False), (4, 0, False), (4, 1, False),
    pytest.param(3, 1, True, marks=pytest.mark.fast)])
def test_tree_at_points(gpu, order, kernel, fast):
    """(e) at points the softening is the source's max(h_j, 0) and there is
    no self skip: a query on a particle of h > 0 is finite; on one of h = 0,
    negative or NaN it follows the Newtonian rule (-m / sqrt(R2_TINY), a
    0 * inf force)."""
    pos, mass, h = tree_inputs()
    ref = tree_ref(order, kernel)[0]
    q = plummer(500, seed=22)[0] * 1.3
    q[:10] = pos[:10]
    soft = np.zeros(500, dtype=bool)
    soft[:10] = h[:10] > 0
    hard = np.zeros(500, dtype=bool)
    hard[:10] = ~soft[:10]
    assert soft.sum() == 7 and hard.sum() == 3  # rows 0 (h = 0), 5 (negative), 7 (NaN)
    bound = FAST if fast else TIGHT
    dev = _engine.Octree(pos, mass, LEAF, order, h, kernel)
    pd, pr = dev.potentials_at_points(q, THETA), ref.potentials_at_points(q, THETA)
    ad, ar = dev.accelerations_at_points(q, THETA), ref.accelerations_at_points(q, THETA)
    assert np.isfinite(pr[~hard]).all() and np.isfinite(ar[~hard]).all()
    check_values(f"at points order {order} kernel {kernel} fast {fast}", pd[~hard], ad[~hard],
                 pr[~hard], ar[~hard], bound)
    check_values("  on particles of h > 0", pd[soft], ad[soft], pr[soft], ar[soft], bound)
    assert np.all(pd[hard] < -1e140) and np.allclose(pd[hard], pr[hard], rtol=bound, atol=0.0)
    assert np.isnan(ar[hard]).any() and np.array_equal(np.isnan(ad[hard]), np.isnan(ar[hard]))
    dev.close()


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("case", ["zero_mass", "cluster_soft", "cluster_hard"])
def test_tree_zero_mass_and_coincident_cluster(gpu, case, kernel):
    """(f) empty subtrees under softening, and 30 particles on one point (more
    than a leaf holds) with h = 0.03 (everything finite) or h = 0 (Newtonian:
    the NaN pattern of the oracle)."""
    if case == "zero_mass":  # the masses of test_gpu_tree.py::test_zero_mass_subtrees
        pos, mass, h = tree_inputs()
        mass = mass.copy()
        mass[pos[:, 0] > 0.3] = 0.0
        mass[::7] = 0.0
        theta = THETA
    else:                    # the particles of test_gpu_tree.py::test_coincident_cluster
        pos = np.random.default_rng(50).random((2000, 3)) - 0.5
        pos[100:130] = pos[100]
        mass = np.ones(2000)
        h = soft_h(2000, 51).copy()
        h[100:130] = 0.03 if case == "cluster_soft" else 0.0
        theta = THETA
    n = len(pos)
    dev = _engine.Octree(pos, mass, LEAF, 3, h, kernel)
    ref = ot.RefOctree(pos, mass, LEAF, 3, softenings=h, kernel=kernel)
    check_structure(dev, ref, 3)
    pot_r, acc_r, nn_r, np_r = ref.compute_subset(np.arange(n), theta)
    pot_d = dev.compute_potentials(theta)
    cnt = dev.info()
    acc_d = dev.compute_accelerations(theta)
    assert cnt["node_interactions"] == int(nn_r.sum()) and cnt["leaf_pairs"] == int(np_r.sum())
    nan_r = np.isnan(acc_r).any(axis=1)
    if case == "cluster_hard":
        assert np.array_equal(np.flatnonzero(nan_r), np.arange(100, 130))
        assert np.array_equal(np.isnan(acc_d), np.isnan(acc_r))
        assert np.all(pot_d[nan_r] < -1e140)
    else:
        assert not nan_r.any() and np.isfinite(pot_r).all()
    ok = ~nan_r
    rp = rel_pot(pot_d, pot_r)
    print(f"{case} kernel {kernel}: pot (all rows) {rp:.2e}")
    assert np.isfinite(pot_d).all() and rp < TIGHT
    check_values(f"{case} kernel {kernel}", pot_d[ok], acc_d[ok], pot_r[ok], acc_r[ok], TIGHT)
    dev.close()


@pytest.mark.fast
def test_tree_shared_record_slot(gpu):
    """(g) slot 5 of a walk record is h_max for a tree built with softenings
    and size2 / theta^2 for the fast unsoftened walk (open_scale).  One handle
    through both uses, every step against a RefOctree driven the same way."""
    pos, mass, h = tree_inputs()
    n = len(pos)
    dev = _engine.Octree(pos, mass, LEAF, 3)
    ref = ot.RefOctree(pos, mass, LEAF, 3)
    nn0, np0 = unsoftened_totals()

    def step(label, theta=THETA):
        pot_r, acc_r, nn_r, np_r = ref.compute_subset(np.arange(n), theta)
        return walk_and_check(label, dev, pot_r, acc_r, nn_r, np_r, theta, FAST)

    # 1. fast unsoftened: the slot holds size2 / theta^2, for two thetas
    pot1, acc1, t1 = step("1 unsoftened 0.5")
    assert t1 == (nn0, np0) and dev.export()["hmax"] is None
    step("1 unsoftened 0.7", 0.7)
    # 2. softenings without a rebuild: softened leaves, no guard (tree.rs:1076)
    for t in (dev, ref):
        t.set_kernel(0)
        t.set_softenings(h)
    pot2, _, t2 = step("2 set_softenings")
    assert t2 == (nn0, np0) and not np.array_equal(pot2, pot1)
    assert dev.export()["hmax"] is None
    # 3. build_mass: h_max written into the slot, the guard on
    for t in (dev, ref):
        t.build_mass()
    check_structure(dev, ref, 3)
    assert dev.export()["hmax"] is not None and ref.export()["hmax"] is not None
    _, _, t3 = step("3 build_mass")
    assert t3[0] <= nn0 - 1000 and t3[1] > np0
    # 4. the other kernel: another separation factor on the same h_max
    for t in (dev, ref):
        t.set_kernel(1)
    _, _, t4 = step("4 set_kernel(1)")
    assert t3[0] <= t4[0] - 1000
    # 5. no softenings: the build-time guard stays (tree.rs:777-782)
    for t in (dev, ref):
        t.set_softenings(None)
    _, _, t5 = step("5 set_softenings(None)")
    assert t5[0] < nn0 and t5[1] > np0
    # 6. a rebuilt payload without softenings: fresh records, the slot must be
    # scaled again even at the theta it was last scaled for (0.7, step 1)
    m2 = 0.5 + np.random.default_rng(13).random(n)
    for t in (dev, ref):
        t.build_mass(m2)
    check_structure(dev, ref, 3)
    assert dev.export()["hmax"] is None
    step("6 build_mass(m2) 0.7", 0.7)
    step("6 build_mass(m2) 0.5")
    # 7. unsoftened again: the first walk's values bit for bit, from this
    # handle with the first masses and from a fresh one
    for t in (dev, ref):
        t.build_mass(np.array(mass))
    pot7, acc7, t7 = step("7 build_mass(mass)")
    assert t7 == t1 and np.array_equal(pot7, pot1) and np.array_equal(acc7, acc1)
    fresh = _engine.Octree(pos, mass, LEAF, 3)
    assert np.array_equal(fresh.compute_potentials(THETA), pot1)
    assert np.array_equal(fresh.compute_accelerations(THETA), acc1)
    fresh.close()
    dev.close()


def test_gravity_front_end_softened(gpu):
    """(h) Gravity(..., softening=0.05, kernel=Spline): tree and direct sums."""
    pos, mass, _ = tree_inputs()
    n = len(pos)
    h = np.full(n, 0.05)
    g = Gravity(pos, mass, softening=0.05, kernel=KernelKind.Spline)
    ref = ot.RefOctree(pos, mass, 8, 3, softenings=h, kernel=1)  # TreeOptions defaults
    check_values("front end tree", g.tree_potentials(theta=THETA), g.tree_accelerations(theta=THETA),
                 ref.compute_potentials(THETA), ref.compute_accelerations(THETA), TIGHT)
    check_values("front end direct", g.direct_potentials(), g.direct_accelerations(),
                 og.direct_potentials(pos, mass, h, 1), og.direct_accelerations(pos, mass, h, 1),
                 DIRECT)


# ---------------------------------------------------------- direct sum
def sym_stats():
    u, g = ctypes.c_int64(), ctypes.c_int64()
    nat.call("pbx_direct_sym_path_stats", ctypes.byref(u), ctypes.byref(g))
    return u.value, g.value


@functools.lru_cache(maxsize=None)
def direct_ref(n, kernel, softened=True):
    """Oracle (pot, acc) of the all-particles form on direct_inputs(n)."""
    pos, mass, h = direct_inputs(n)
    hh = h if softened else None
    return frozen(og.direct_potentials(pos, mass, hh, kernel),
                  og.direct_accelerations(pos, mass, hh, kernel))


def check_direct(label, pot_d, acc_d, pot_r, acc_r, bound=DIRECT, nan_rows=None):
    """NaN where the reference is NaN (``nan_rows``: and nowhere else than
    there), the other rows finite and within the contract and ``bound``."""
    nan_p, nan_a = np.isnan(pot_r), np.isnan(acc_r)
    if nan_rows is not None:
        assert np.array_equal(nan_p, nan_rows)
    assert np.array_equal(np.isnan(pot_d), nan_p) and np.array_equal(np.isnan(acc_d), nan_a)
    okp, oka = ~nan_p, ~nan_a.any(axis=1)
    assert np.isfinite(pot_d[okp]).all() and np.isfinite(acc_d[oka]).all()
    rp, ra = rel_pot(pot_d[okp], pot_r[okp]), rel_acc(acc_d[oka], acc_r[oka])
    print(f"{label}: pot {rp:.2e} acc {ra:.2e} ({int(nan_p.sum())} NaN rows)")
    assert rp < TOL and ra < TOL
    assert rp < bound and ra < bound, (rp, ra)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("n", [4097, 8192, 9000])
def test_direct_source_splits(gpu, n, kernel):
    """(i) 2, 2 and 3 source splits: the diagonal window of a target tile
    clamped against a split, partial slabs, reduce_splits — with a kernel.
    The rows of NaN softening see each other: NaN, as in the reference."""
    pos, mass, h = direct_inputs(n)
    before = sym_stats()
    pot = _engine.direct_potentials_py(pos, mass, 0, h, kernel)
    acc = _engine.direct_accelerations_py(pos, mass, 0, h, kernel)
    assert sym_stats() == before
    check_direct(f"splits n {n} kernel {kernel}", pot, acc, *direct_ref(n, kernel),
                 nan_rows=np.isnan(h))


def test_direct_kernel_stays_off_symmetric_path(gpu):
    """(j) direct_sym.hip is Newtonian only: at n >= 8192 a call that carries
    a kernel, with or without softenings, must not be routed there."""
    n = 9000
    pos, mass, h = direct_inputs(n)
    pot_n, acc_n = og.direct_potentials(pos, mass), og.direct_accelerations(pos, mass)
    for kernel in (0, 1):
        before = sym_stats()
        pot = _engine.direct_potentials_py(pos, mass, 0, None, kernel)
        acc = _engine.direct_accelerations_py(pos, mass, 0, None, kernel)
        assert sym_stats() == before
        # h = 0 everywhere: the Newtonian sum, and not at the symmetric path's fast precision
        check_direct(f"kernel {kernel} no softenings", pot, acc, pot_n, acc_n)
        _engine.direct_potentials_py(pos, mass, 0, h, kernel)
        assert sym_stats() == before
    before = sym_stats()
    _engine.direct_potentials_py(pos, mass)
    after = sym_stats()
    assert sum(after) > sum(before) and after[0] >= before[0] and after[1] >= before[1]


@pytest.mark.parametrize("kernel", [None, 0, 1])
@pytest.mark.parametrize("m", [1, 1025])
def test_direct_at_points_tails(gpu, m, kernel):
    """(k) 4097 sources (two splits) at 1 and 1025 targets: a target tile
    with a tail, clamped target loads."""
    pos, mass, h = direct_inputs(4097)
    hh = None if kernel is None else h
    tgt = plummer(m, seed=41 + m)[0] * 1.2
    pot = _engine.direct_potentials_at_points_py(pos, tgt, mass, 0, hh, kernel)
    acc = _engine.direct_accelerations_at_points_py(pos, tgt, mass, 0, hh, kernel)
    check_direct(f"at points m {m} kernel {kernel}", pot, acc,
                 og.direct_potentials_at_points(pos, tgt, mass, hh, kernel),
                 og.direct_accelerations_at_points(pos, tgt, mass, hh, kernel),
                 nan_rows=np.zeros(m, dtype=bool))


@pytest.mark.parametrize("kernel", [0, 1])
def test_direct_against_longdouble(gpu, kernel):
    """(l) the second yardstick: no operation order shared with the kernel."""
    pos, mass, h = direct_inputs(600)
    pot = _engine.direct_potentials_py(pos, mass, 0, h, kernel)
    acc = _engine.direct_accelerations_py(pos, mass, 0, h, kernel)
    check_direct(f"long double kernel {kernel} all particles", pot, acc,
                 *direct_longdouble(pos, mass, h, kernel), nan_rows=np.isnan(h))
    tgt = plummer(130, seed=43)[0] * 1.2
    pot = _engine.direct_potentials_at_points_py(pos, tgt, mass, 0, h, kernel)
    acc = _engine.direct_accelerations_at_points_py(pos, tgt, mass, 0, h, kernel)
    check_direct(f"long double kernel {kernel} at points", pot, acc,
                 *direct_longdouble(pos, mass, h, kernel, tgt), nan_rows=np.zeros(130, dtype=bool))


@pytest.mark.parametrize("single_nan", [False, True], ids=["nan_rows", "one_nan_row"])
@pytest.mark.parametrize("kernel", [0, 1])
def test_direct_softening_edge_values(gpu, kernel, single_nan):
    """(m) 0, negative and NaN softenings, coincident pairs (see
    _soft_data.edge_inputs).  One NaN row alone stays finite: only a pair of
    two NaN softenings is NaN, and a particle is no pair with itself."""
    pos, mass, h, tgt = edge_inputs(single_nan)
    pot = _engine.direct_potentials_py(pos, mass, 0, h, kernel)
    acc = _engine.direct_accelerations_py(pos, mass, 0, h, kernel)
    pot_r = og.direct_potentials(pos, mass, h, kernel)
    acc_r = og.direct_accelerations(pos, mass, h, kernel)
    check_direct(f"edges kernel {kernel} single_nan {single_nan} all particles", pot, acc, pot_r,
                 acc_r, nan_rows=np.zeros(300, dtype=bool) if single_nan else np.isnan(h))
    # the coincident pair softened by one of its two: finite, the oracle's
    assert np.isfinite(pot[[20, 21]]).all() and np.isfinite(acc[[20, 21]]).all()
    assert rel_pot(pot[[20, 21]], pot_r[[20, 21]]) < DIRECT
    assert rel_acc(acc[[20, 21]], acc_r[[20, 21]]) < DIRECT
    # the unsoftened coincident pair: Newtonian, 0 * inf
    assert np.all(pot[[30, 31]] < -1e140) and np.isnan(acc[[30, 31]]).any(axis=1).all()
    # the close pair of two negative softenings
    assert rel_pot(pot[[5, 6]], pot_r[[5, 6]]) < DIRECT and rel_acc(acc[[5, 6]], acc_r[[5, 6]]) < DIRECT
    pot = _engine.direct_potentials_at_points_py(pos, tgt, mass, 0, h, kernel)
    acc = _engine.direct_accelerations_at_points_py(pos, tgt, mass, 0, h, kernel)
    pot_r = og.direct_potentials_at_points(pos, tgt, mass, h, kernel)
    acc_r = og.direct_accelerations_at_points(pos, tgt, mass, h, kernel)
    check_direct(f"edges kernel {kernel} single_nan {single_nan} at points", pot, acc, pot_r, acc_r,
                 nan_rows=np.zeros(len(tgt), dtype=bool))
    assert np.isfinite(acc[0]).all() and pot[0] > -1e3
    assert np.all(pot[1:4] < -1e140) and np.isnan(acc[1:4]).any(axis=1).all()


@pytest.mark.parametrize("kernel", [nat.KERNEL_NONE, 0, 1])
def test_direct_device_shard(gpu, kernel):
    """(n) pbx_direct_dev as a rank of a sharded solve calls it: targets
    [3001, 6002) of 9000 sources, self offset 3001, three source splits,
    softenings of sources and targets on the device, potential and
    acceleration in one launch — the same rows of the full oracle solve."""
    n, lo, hi = 9000, 3001, 6002
    pos, mass, h = direct_inputs(n)
    m = hi - lo
    d_pos, d_mass = nat.DeviceArray.from_host(pos), nat.DeviceArray.from_host(mass)
    d_rec = nat.DeviceArray(32 * n)
    nat.call("pbx_pack_sources", d_pos.ptr, d_mass.ptr, n, d_rec.ptr)
    d_h = nat.DeviceArray.from_host(h)
    d_tgt = nat.DeviceArray.from_host(np.ascontiguousarray(pos[lo:hi]))
    d_tgt_h = nat.DeviceArray.from_host(np.ascontiguousarray(h[lo:hi]))
    d_out_p, d_out_a = nat.DeviceArray(8 * m), nat.DeviceArray(24 * m)
    before = sym_stats()
    nat.call("pbx_direct_dev", d_rec.ptr, d_h.ptr, n, d_tgt.ptr, d_tgt_h.ptr, m, lo, kernel, 3,
             d_out_p.ptr, d_out_a.ptr)
    pot = d_out_p.download(np.empty(m))
    acc = d_out_a.download(np.empty((m, 3)))
    assert sym_stats() == before  # a non-zero offset is no symmetric solve, with any kernel
    if kernel == nat.KERNEL_NONE:
        pot_r, acc_r = og.direct_subset(pos, mass, np.arange(lo, hi))
        nan_rows = np.zeros(m, dtype=bool)
    else:
        pot_r, acc_r = (x[lo:hi] for x in direct_ref(n, kernel))
        nan_rows = np.isnan(h[lo:hi])
    check_direct(f"device shard kernel {kernel}", pot, acc, pot_r, acc_r, nan_rows=nan_rows)
    for a in (d_pos, d_mass, d_rec, d_h, d_tgt, d_tgt_h, d_out_p, d_out_a):
        a.free()
