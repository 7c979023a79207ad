"""Pin the yardsticks and the inputs of tests/test_gpu_softened.py — CPU only.

  * the C oracle's softened direct sums (oracle/gravity_ref.c) against
    ``_soft_data.direct_longdouble``, a whole-array long-double restatement
    of direct.rs / kernel.rs that shares neither code nor operation order
    with it: 1e-12 (measured 2e-15 .. 5e-15, printed);
  * the tree inputs make the h_max guard (node_soft_ok, tree.rs:56-71) fire:
    with softenings the oracle accepts thousands of nodes fewer and sums more
    leaf pairs than without, for both kernels — a walk that ignored h_max, or
    used the other kernel's separation factor, cannot reach the same counts;
  * the direct-sum inputs put at least 100 pairs into each branch of the
    spline (u < 0.5, 0.5 <= u < 1, u >= 1);
  * the edge inputs mean what the GPU test says they mean.
"""
import numpy as np
import pytest

from oracle import gravity as og
from oracle import tree as ot
from pynbodyext.synthetic import plummer

from _soft_data import (DIRECT_SIZES, NAN_ROWS, direct_inputs, direct_longdouble, edge_inputs,
                        soft_h, spline_branch_counts, tree_inputs)

YARDSTICK = 1e-12


def rel_pot(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def rel_acc(a, b):
    return float(np.max(np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)))


def test_soft_h_rows():
    h = soft_h(6000, 12)
    assert not h.flags.writeable and soft_h(6000, 12) is h
    kind = np.zeros(6000, dtype=int)  # written in this order: a later row wins
    kind[::97] = 1
    kind[5::101] = 2
    kind[7::103] = 3
    assert np.all(h[kind == 1] == 0.0) and np.all(h[kind == 2] == -0.01)
    assert np.all(np.isnan(h[kind == 3]))
    assert [int((kind == k).sum()) for k in (1, 2, 3)] == [60, 60, 59]
    rest = kind == 0
    assert np.all(h[rest] > 0) and np.isfinite(h[rest]).all()
    assert 0.015 < np.median(h[rest]) < 0.025
    assert h[rest].max() / h[rest].min() > 1e3  # sigma 1.2: three decades at n = 6000


@pytest.mark.parametrize("kernel", [0, 1])
def test_oracle_against_longdouble(kernel):
    """n = 400 Plummer sphere, soft_h, a coincident pair with h = 0.03.

    All-particles form: the softening of a pair is the plain hi.max(hj) of
    direct.rs:395,472 — NaN when both are NaN — so the rows of NaN softening
    (four of them here, each seeing three others) are NaN in the reference,
    in the oracle and in the long-double sum alike; every other row, the
    coincident pair included, is finite.  At points (max(h_j, 0)) everything
    is finite, the query on top of the coincident pair included."""
    pos, mass = plummer(400, seed=3)
    h = soft_h(400, 4).copy()
    pos[51] = pos[50]
    h[50] = h[51] = 0.03
    nan_rows = np.zeros(400, dtype=bool)
    nan_rows[NAN_ROWS] = True
    assert nan_rows.sum() == 4

    pot_o = og.direct_potentials(pos, mass, h, kernel)
    acc_o = og.direct_accelerations(pos, mass, h, kernel)
    pot_l, acc_l = direct_longdouble(pos, mass, h, kernel)
    for p, a in ((pot_o, acc_o), (pot_l, acc_l)):
        assert np.array_equal(np.isnan(p), nan_rows)
        assert np.array_equal(np.isnan(a).any(axis=1), nan_rows)
        assert np.isfinite(p[~nan_rows]).all() and np.isfinite(a[~nan_rows]).all()
    ok = ~nan_rows
    rp, ra = rel_pot(pot_o[ok], pot_l[ok]), rel_acc(acc_o[ok], acc_l[ok])
    print(f"kernel {kernel} all-particles: pot {rp:.2e} acc {ra:.2e}")
    assert rp <= YARDSTICK and ra <= YARDSTICK

    tgt = plummer(120, seed=5)[0] * 1.2
    tgt[0] = pos[50]
    pot_o = og.direct_potentials_at_points(pos, tgt, mass, h, kernel)
    acc_o = og.direct_accelerations_at_points(pos, tgt, mass, h, kernel)
    pot_l, acc_l = direct_longdouble(pos, mass, h, kernel, tgt)
    for x in (pot_o, acc_o, pot_l, acc_l):
        assert np.isfinite(x).all()
    rp, ra = rel_pot(pot_o, pot_l), rel_acc(acc_o, acc_l)
    print(f"kernel {kernel} at points:     pot {rp:.2e} acc {ra:.2e}")
    assert rp <= YARDSTICK and ra <= YARDSTICK


def test_longdouble_newtonian_limit():
    """direct_longdouble without softenings is the Newtonian oracle."""
    pos, mass = plummer(300, seed=9)
    for kernel in (0, 1):
        pot, acc = direct_longdouble(pos, mass, None, kernel)
        assert rel_pot(og.direct_potentials(pos, mass), pot) <= YARDSTICK
        assert rel_acc(og.direct_accelerations(pos, mass), acc) <= YARDSTICK


def _counts(order, kernel, h):
    pos, mass, _ = tree_inputs()
    ref = ot.RefOctree(pos, mass, 8, order, softenings=h, kernel=kernel)
    pot, acc, nn, npairs = ref.compute_subset(np.arange(len(pos)), 0.5)
    assert not np.isnan(pot).any() and not np.isnan(acc).any()
    return int(nn.sum()), int(npairs.sum())


def test_guard_fires():
    """Measured at order 3 (and, the same, at order 0): unsoftened 787 468
    accepted nodes / 10 975 636 leaf pairs; Plummer 778 323 / 12 259 475;
    spline 784 092 / 11 024 250."""
    h = tree_inputs()[2]
    nn0, np0 = _counts(3, None, None)
    print(f"unsoftened: {nn0} accepted nodes, {np0} leaf pairs")
    seen = {}
    for kernel in (0, 1):
        nn, npairs = _counts(3, kernel, h)
        print(f"kernel {kernel}:   {nn} accepted nodes, {npairs} leaf pairs")
        assert nn <= nn0 - 1000 and npairs > np0
        seen[kernel] = (nn, npairs)
        assert _counts(0, kernel, h) == (nn, npairs)  # the decisions do not depend on the order
    # the two separation factors (2.8, 1.0) decide differently
    assert seen[0][0] <= seen[1][0] - 1000


@pytest.mark.parametrize("n", DIRECT_SIZES)
def test_spline_branches_populated(n):
    pos, _, h = direct_inputs(n)
    # (n >= 4097: the pairs of the first 1024 particles are enough, a lower bound)
    inner, mid, outer = spline_branch_counts(pos, h, max_rows=1024)
    print(f"n {n}: u < 0.5: {inner}, 0.5 <= u < 1: {mid}, u >= 1: {outer}")
    assert min(inner, mid, outer) >= 100


@pytest.mark.parametrize("single_nan", [False, True])
@pytest.mark.parametrize("kernel", [0, 1])
def test_edge_inputs_mean_what_they_say(kernel, single_nan):
    pos, mass, h, tgt = edge_inputs(single_nan)
    assert h[5] < 0 and h[6] < 0 and np.linalg.norm(pos[5] - pos[6]) < 0.01
    assert np.isnan(h[7]) and np.isnan(h).sum() == (1 if single_nan else 3)
    inner, mid, outer = spline_branch_counts(pos, h)
    assert min(inner, mid, outer) >= 100
    pot = og.direct_potentials(pos, mass, h, kernel)
    acc = og.direct_accelerations(pos, mass, h, kernel)
    nan_rows = np.zeros(300, dtype=bool) if single_nan else np.isnan(h)
    assert np.array_equal(np.isnan(pot), nan_rows)
    acc_nan = nan_rows.copy()
    acc_nan[[30, 31]] = True  # coincident and unsoftened: (m * 0) * inf
    assert np.array_equal(np.isnan(acc).any(axis=1), acc_nan)
    assert np.isfinite(pot[[20, 21]]).all() and np.all(pot[[20, 21]] > -1e3)
    assert np.all(pot[[30, 31]] < -1e140)
    pot_l, acc_l = direct_longdouble(pos, mass, h, kernel)
    ok = ~acc_nan
    assert rel_pot(pot[ok], pot_l[ok]) <= YARDSTICK and rel_acc(acc[ok], acc_l[ok]) <= YARDSTICK
    # at points: max(h_j, 0)
    pot = og.direct_potentials_at_points(pos, tgt, mass, h, kernel)
    acc = og.direct_accelerations_at_points(pos, tgt, mass, h, kernel)
    assert np.isfinite(pot[0]) and pot[0] > -1e3 and np.isfinite(acc[0]).all()
    assert np.all(pot[1:4] < -1e140) and np.isnan(acc[1:4]).any(axis=1).all()
    assert np.isfinite(pot[4:]).all() and np.isfinite(acc[4:]).all()
