"""Inputs and an independent yardstick for the multipole tests of the
Barnes–Hut tree (tests/test_oracle_multipole.py on the CPU,
tests/test_gpu_multipole.py on the GPU).  No tests in here.

The yardstick is the textbook Legendre series of 1/|x - y| about a node's
centre of mass, summed particle by particle in ``np.longdouble``.  It shares
no arithmetic with oracle/tree_ref.c (Cartesian moment and derivative
tensors) nor with csrc/tree.hip (detraced tensors, binomial P2M, butterfly
M2M); the oracle is only asked for the *tree* (``RefOctree.export()``: links,
leaf lists, sizes and the float64 centres of mass the moments refer to).

Conventions (each one breaks equality when guessed wrong; pinned by
tests/test_oracle_multipole.py):

  eo = 0 if order <= 1 else min(order, 5)     order 1 is stored as order 0
  s_i = x_i - com, d = target - com, u_i = s_i^ . d^   (com: exported float64)
  potential of an accepted node
      - sum_{k <= eo, k != 1} sum_i m_i |s_i|^k P_k(u_i) / |d|^(k+1)
  acceleration of an accepted node: the gradient series through
      k <= max(eo - 1, 0)  (the walk builds derivative tensors to order eo
      only, one of which the gradient uses up), per term
      sum_i m_i |s_i|^k [P_k'(u_i) (s_i^ - u_i d^) - (k+1) P_k(u_i) d^] / |d|^(k+2)
  the k = 1 term is the rounding residue of the dipole about the centre of
      mass: the potential evaluators drop it, the acceleration evaluator of
      the oracle contracts it with the second derivatives, so it is kept
      there (2 * eps * |com| / |d| of the monopole: 3.5e-13 where the
      coordinates are 2300 edges);
  walk: from node 0, nodes of mass 0 skipped, a leaf summed particle by
      particle (without ``skip``), an internal node accepted iff
      size2 < theta^2 * dist2 (strict), else descended.
"""
import functools
from math import factorial

import numpy as np

L = np.longdouble
KMAX = 5
THETAS = (0.5, 0.9)
ORDERS = (0, 1, 2, 3, 4, 5)
SHELLS = (1.0, 1.5, 3.0)
SHELL_THETA = 1.5
N_SHELL = 40
MIN_MARGIN = 1e-9
CANCEL_MAX = 20.0    # sum |a_j| / |sum a_j| above which a particle is no target

# (l, m, n) of the 56 moment slots in the oracle's order, pinned by
# m[4] = 1/2 sum x^2 and m[20] = sum x^4 / 24 (test_oracle_multipole.py)
LMN = (
    (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1),
    (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (1, 0, 1), (0, 1, 1),
    (3, 0, 0), (0, 3, 0), (0, 0, 3), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 0, 2), (0, 2, 1),
    (0, 1, 2), (1, 1, 1),
    (4, 0, 0), (0, 4, 0), (0, 0, 4), (3, 1, 0), (3, 0, 1), (1, 3, 0), (1, 0, 3), (0, 3, 1),
    (0, 1, 3), (2, 2, 0), (2, 0, 2), (0, 2, 2), (2, 1, 1), (1, 2, 1), (1, 1, 2),
    (5, 0, 0), (0, 5, 0), (0, 0, 5), (4, 1, 0), (4, 0, 1), (1, 4, 0), (1, 0, 4), (0, 4, 1),
    (0, 1, 4), (3, 2, 0), (3, 0, 2), (2, 3, 0), (2, 0, 3), (0, 3, 2), (0, 2, 3), (2, 2, 1),
    (2, 1, 2), (1, 2, 2), (3, 1, 1), (1, 3, 1), (1, 1, 3),
)
DEG = np.array([sum(t) for t in LMN])
NCOEF = {0: 1, 1: 4, 2: 10, 3: 20, 4: 35, 5: 56}


def eo_of(order):
    return 0 if order <= 1 else min(order, KMAX)


# ------------------------------------------------------------- the series
def legendre(k, u):
    """(P_k(u), P_k'(u)) in long double:
    (n+1) P_{n+1} = (2n+1) u P_n - n P_{n-1},  P'_{n+1} = P'_{n-1} + (2n+1) P_n."""
    u = np.asarray(u, dtype=L)
    p_prev, p = np.ones_like(u), u.copy()
    d_prev, d = np.zeros_like(u), np.ones_like(u)
    if k == 0:
        return p_prev, d_prev
    for n in range(1, k):
        p_prev, p = p, ((2 * n + 1) * u * p - n * p_prev) / (n + 1)
        d_prev, d = d, d_prev + (2 * n + 1) * p_prev
    return p, d


def node_series(pos, mass, com, target, kmax=KMAX, swap_yz=False):
    """Per-order terms (phi[k], acc[k, 3]), k = 0..kmax, of the particles
    (pos, mass) seen from ``target`` in the Legendre series about ``com``.
    ``com`` may be one centre or one per particle (the accepted nodes of a
    walk side by side: their terms add).  ``swap_yz`` is the planted error
    of the sensitivity test (y and z of s_i exchanged)."""
    p = np.asarray(pos, dtype=L).reshape(-1, 3)
    m = np.asarray(mass, dtype=L)
    c = np.broadcast_to(np.asarray(com, dtype=L), p.shape)
    s = p - c
    if swap_yz:
        s = s[:, [0, 2, 1]]
    d = np.asarray(target, dtype=L) - c
    dn = np.sqrt((d * d).sum(axis=1))
    dh = d / dn[:, None]
    sn = np.sqrt((s * s).sum(axis=1))
    sh = s / np.where(sn > 0, sn, L(1))[:, None]
    u = (sh * dh).sum(axis=1)
    phi = np.zeros(kmax + 1, dtype=L)
    acc = np.zeros((kmax + 1, 3), dtype=L)
    w = m.copy()          # m |s|^k
    inv = 1 / dn          # 1 / |d|^(k+1)
    for k in range(kmax + 1):
        P, dP = legendre(k, u)
        phi[k] = -(w * P * inv).sum()
        vec = dP[:, None] * (sh - u[:, None] * dh) - (k + 1) * P[:, None] * dh
        acc[k] = ((w * inv / dn)[:, None] * vec).sum(axis=0)
        w = w * sn
        inv = inv / dn
    return phi, acc


def combine(phi_terms, acc_terms, order, drop_top=False, scale_top=1.0, acc_through_eo=False):
    """Sum the per-order node terms as the evaluators of ``order`` do.  The
    keywords are the planted errors 1-3 of the sensitivity test."""
    eo = eo_of(order)
    ka = eo if acc_through_eo else max(eo - 1, 0)
    phi = L(0)
    for k in range(eo + 1):
        if k == 1 or (drop_top and k == eo):
            continue
        phi = phi + phi_terms[..., k] * (L(scale_top) if k == eo else L(1))
    acc = sum(acc_terms[..., k, :] for k in range(ka + 1))
    return phi, acc


def p2m(pos, mass, center):
    """Raw moments sum m s_x^a s_y^b s_z^c / (a! b! c!) about ``center`` in
    long double, in the order of ``LMN``."""
    s = np.asarray(pos, dtype=L).reshape(-1, 3) - np.asarray(center, dtype=L)
    m = np.asarray(mass, dtype=L)
    out = np.zeros(len(LMN), dtype=L)
    for i, (a, b, c) in enumerate(LMN):
        out[i] = (m * s[:, 0] ** a * s[:, 1] ** b * s[:, 2] ** c).sum() / \
            (factorial(a) * factorial(b) * factorial(c))
    return out


def leaf_sum(pos, mass, target):
    """(phi, acc, sum of |a_i|) of a direct sum in long double."""
    d = np.asarray(pos, dtype=L).reshape(-1, 3) - np.asarray(target, dtype=L)
    m = np.asarray(mass, dtype=L)
    r2 = (d * d).sum(axis=1)
    r = np.sqrt(r2)
    return -(m / r).sum(), ((m / (r2 * r))[:, None] * d).sum(axis=0), (m / r2).sum()


# --------------------------------------------------------------- the walk
def node_particles(export, k):
    """Original indices of the particles under node k: follow first/next
    from first[k] until next[k]."""
    if export["leaf_off"][k] >= 0:
        o = export["leaf_off"][k]
        return export["perm"][o:o + export["leaf_len"][k]]
    first, nxt, off, cnt = export["first"], export["next"], export["leaf_off"], export["leaf_len"]
    out, j, stop = [], first[k], nxt[k]
    while j != stop:
        if off[j] >= 0:
            out.append(export["perm"][off[j]:off[j] + cnt[j]])
            j = nxt[j]
        else:
            j = first[j]
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


class WalkTree:
    """A tree in the shape of ``RefOctree.export()`` with its particles,
    walked in long double."""

    def __init__(self, export, pos, mass):
        self.e = export
        self.pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
        self.mass = np.asarray(mass, dtype=np.float64)
        self.first = export["first"].tolist()
        self.next = export["next"].tolist()
        self.leaf = (export["leaf_off"] >= 0).tolist()
        self.empty = (export["mass"] == 0.0).tolist()
        self.com = export["com"].astype(L)
        self.size2 = export["size2"].astype(L)
        self._ids = {}

    def ids(self, k):
        if k not in self._ids:
            self._ids[k] = node_particles(self.e, k)
        return self._ids[k]

    def terms(self, theta, target, skip=-1, accept_equal=False, swap_yz=False):
        """One target's walk: (phi_leaf, acc_leaf, phi_terms[6], acc_terms[6, 3],
        accepted nodes, leaf particles, minimum decision margin, sum of the
        magnitudes of the leaf pairs' and node monopoles' accelerations).  ``accept_equal`` is planted error 5
        (<= in the opening test)."""
        t = np.asarray(target, dtype=L)
        theta2 = L(np.float64(theta) * np.float64(theta))
        d = self.com - t
        bound = theta2 * (d * d).sum(axis=1)
        with np.errstate(all="ignore"):
            margin = np.abs(self.size2 / bound - 1)
        ok = ((self.size2 <= bound) if accept_equal else (self.size2 < bound)).tolist()
        nodes, leaves, decided = [], [], []
        k = 0
        while k != -1:
            if self.empty[k]:
                k = self.next[k]
            elif self.leaf[k]:
                leaves.append(k)
                k = self.next[k]
            else:
                decided.append(k)
                if ok[k]:
                    nodes.append(k)
                    k = self.next[k]
                else:
                    k = self.first[k]
        lid = np.concatenate([self.ids(k) for k in leaves]) if leaves else np.zeros(0, np.int64)
        n_leaf = len(lid)
        lid = lid[lid != skip]
        phi_leaf, acc_leaf, asum = leaf_sum(self.pos[lid], self.mass[lid], t)
        if nodes:
            nid = np.concatenate([self.ids(k) for k in nodes])
            com = np.concatenate([np.broadcast_to(self.com[k], (len(self.ids(k)), 3))
                                  for k in nodes])
            phi_t, acc_t = node_series(self.pos[nid], self.mass[nid], com, t, KMAX, swap_yz)
            asum = asum + (self.e["mass"][nodes] / (d[nodes] ** 2).sum(axis=1)).sum()
        else:
            phi_t, acc_t = np.zeros(KMAX + 1, dtype=L), np.zeros((KMAX + 1, 3), dtype=L)
        mm = float(margin[decided].min()) if decided else np.inf
        return phi_leaf, acc_leaf, phi_t, acc_t, len(nodes), n_leaf, mm, float(asum)


def reference_walk(export, order, theta, target, skip, pos, mass, **planted):
    """(phi, acc, n_nodes, n_leaf_particles, min_decision_margin) of one
    target; ``skip`` is the target's own index or -1.  ``planted``: the
    errors of the sensitivity test (accept_equal, swap_yz, drop_top,
    scale_top, acc_through_eo)."""
    walk = {k: planted.pop(k) for k in ("accept_equal", "swap_yz") if k in planted}
    pl, al, pt, at, nn, npp, mm, _ = WalkTree(export, pos, mass).terms(theta, target, skip, **walk)
    phi, acc = combine(pt, at, order, **planted)
    return phi + pl, acc + al, nn, npp, mm


# ----------------------------------------------------------------- inputs
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


OFFSET = np.array([1000.0, -2000.0, 500.0])

# (name, leaf capacity) of every tree of the tests
CASES = (("cube", 8), ("plummer", 8), ("rod_x", 8), ("rod_y", 8), ("rod_z", 8), ("rod_d", 8),
         ("rod_x", 1), ("rod_y", 1), ("rod_z", 1), ("rod_d", 1), ("shifted", 8), ("two_scale", 8))
CASE_IDS = tuple(f"{n}-leaf{c}" for n, c in CASES)
SHELL_CASES = tuple(c for c in CASES if c[1] == 8)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(pos, mass), read-only.
    cube       600 particles uniform in the unit cube, masses 0.5 + U;
    plummer    3000-particle Plummer sample, masses (0.5 + U) / n, every 97th
               mass 0 and the octant x, y, z > 0 zeroed (empty subtrees);
    rod_x/y/z  300 particles on one axis, rod_d on the body diagonal: one
               family of moment components each; the masses are heavy in
               the first 5% of the rod, moderate in the last 10% and light
               between, so that the top term of every order is a fifth of
               the root's potential or more at |d| = 1 edge on the diagonal
               (the 1.001 scaling of the sensitivity test then shows above
               the fast-mode bound);
    shifted    the cube moved by (1000, -2000, 500) edges;
    two_scale  a 200-particle clump 1e-3 wide inside a unit cloud of 1000."""
    if name == "cube":
        rng = np.random.default_rng(2101)
        return _frozen(rng.random((600, 3)), 0.5 + rng.random(600))
    if name == "shifted":
        pos, mass = inputs("cube")
        return _frozen(pos + OFFSET, mass.copy())
    if name == "plummer":
        from pynbodyext.synthetic import plummer

        pos, _ = plummer(3000, seed=2102)
        mass = (0.5 + np.random.default_rng(2103).random(3000)) / 3000
        mass[::97] = 0.0
        mass[(pos > 0).all(axis=1)] = 0.0
        return _frozen(pos, mass)
    if name.startswith("rod_"):
        axis = name[-1]
        rng = np.random.default_rng(2104 + "xyzd".index(axis))
        t = np.sort(rng.random(300))
        pos = np.zeros((300, 3))
        for c in ((0, 1, 2) if axis == "d" else ("xyz".index(axis),)):
            pos[:, c] = t
        mass = (0.5 + rng.random(300)) * np.where(t < 0.05, 20.0, np.where(t > 0.9, 2.0, 0.05))
        return _frozen(pos, mass)
    if name == "two_scale":
        rng = np.random.default_rng(2109)
        pos = rng.random((1200, 3))
        pos[:200] = np.array([0.3, 0.6, 0.45]) + 1e-3 * (rng.random((200, 3)) - 0.5)
        return _frozen(pos, 0.5 + rng.random(1200))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref_tree(name, leaf):
    """(RefOctree, export, WalkTree): the oracle is asked for the tree only
    (order 0: no moments), the arithmetic is WalkTree's."""
    from oracle import tree as ot

    pos, mass = inputs(name)
    ref = ot.RefOctree(pos, mass, leaf, 0)
    e = ref.export()
    return ref, e, WalkTree(e, pos, mass)


_rows = {}  # (name, leaf, theta, particle) -> WalkTree.terms(...)


def _walk_row(name, leaf, theta, i):
    key = (name, leaf, theta, int(i))
    if key not in _rows:
        _rows[key] = ref_tree(name, leaf)[2].terms(theta, inputs(name)[0][i], int(i))
    return _rows[key]


def _cancellation(row):
    """Largest, over the orders, of sum |a_j| / |sum a_j| of one walk: the
    magnitudes of its leaf pairs' and node monopoles' accelerations over the
    acceleration it adds up to."""
    out = 0.0
    for order in ORDERS:
        _, acc = combine(row[2], row[3], order)
        acc = acc + row[1]
        out = max(out, float(row[7] / np.sqrt((acc * acc).sum())))
    return out


@functools.lru_cache(maxsize=None)
def self_targets(name):
    """64 particle indices: the 16 innermost, the 16 outermost (distance from
    the centre of mass) and 32 random others, among the well-conditioned
    particles.  A particle between two equal neighbours on a rod feels almost
    nothing, and the relative error of its acceleration is the rounding of
    one interaction times sum |a_j| / |sum a_j|: that says nothing about the
    code.  The fast mode's unrefined reciprocal square root is good to ~5e-8
    per interaction (tests/test_gpu_tree.py), so a target is taken only if no
    reference walk of it, at any tree, theta or order of the tests, cancels
    by more than CANCEL_MAX = 20 (1e-6 then, half the fast-mode bound).  The
    rule looks at the long-double series alone."""
    pos, mass = inputs(name)
    leaves = [leaf for n, leaf in CASES if n == name]

    def good(i):
        return all(_cancellation(_walk_row(name, leaf, theta, i)) <= CANCEL_MAX
                   for leaf in leaves for theta in THETAS)

    def take(candidates, count, taken):
        out = []
        for i in candidates:
            if len(out) == count:
                break
            if int(i) not in taken and good(i):
                out.append(int(i))
        assert len(out) == count
        return out

    com = (pos * mass[:, None]).sum(axis=0) / mass.sum()
    by_r = np.argsort(((pos - com) ** 2).sum(axis=1), kind="stable")
    inner = take(by_r, 16, set())
    outer = take(by_r[::-1], 16, set(inner))
    pick = take(np.random.default_rng(2110).permutation(len(pos)), 32, set(inner + outer))
    idx = np.array(pick + inner + outer, dtype=np.int64)
    assert len(np.unique(idx)) == 64
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def shell_targets(name):
    """(SHELLS, N_SHELL, 3) points at SHELLS x root edge from the root's
    centre of mass: the axes, the body diagonal and random directions."""
    _, e, _ = ref_tree(name, 8)
    rng = np.random.default_rng(2111)
    v = rng.normal(size=(N_SHELL, 3))
    v[:6] = np.concatenate([np.eye(3), -np.eye(3)])
    v[6], v[7] = (1.0, 1.0, 1.0), (-1.0, -1.0, -1.0)
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    edge = 2.0 * e["half"][0]
    out = e["com"][0] + np.array(SHELLS)[:, None, None] * edge * v[None]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def walk_terms(name, leaf, theta, swap_yz=False):
    """The 64 self-target walks of one tree, order-independent: dict of
    phi_leaf (64), acc_leaf (64, 3), phi_terms (64, 6), acc_terms (64, 6, 3),
    nodes, leaf_particles (64 int), margin, asum (64).  Read-only, shared."""
    if swap_yz:
        wt, pos = ref_tree(name, leaf)[2], inputs(name)[0]
        rows = [wt.terms(theta, pos[i], int(i), swap_yz=True) for i in self_targets(name)]
    else:
        rows = [_walk_row(name, leaf, theta, i) for i in self_targets(name)]
    out = dict(phi_leaf=np.array([r[0] for r in rows], dtype=L),
               acc_leaf=np.array([r[1] for r in rows], dtype=L),
               phi_terms=np.array([r[2] for r in rows], dtype=L),
               acc_terms=np.array([r[3] for r in rows], dtype=L),
               nodes=np.array([r[4] for r in rows]), leaf_particles=np.array([r[5] for r in rows]),
               margin=np.array([r[6] for r in rows]), asum=np.array([r[7] for r in rows]))
    _frozen(*out.values())
    return out


def walk_values(name, leaf, theta, order, swap_yz=False, **planted):
    """(phi (64), acc (64, 3)) in long double of the self-target walks."""
    w = walk_terms(name, leaf, theta, swap_yz)
    phi, acc = combine(w["phi_terms"], w["acc_terms"], order, **planted)
    return phi + w["phi_leaf"], acc + w["acc_leaf"]


@functools.lru_cache(maxsize=None)
def shell_terms(name, swap_yz=False):
    """Per-order terms (3 * N_SHELL, 6) and (3 * N_SHELL, 6, 3) of all
    particles about the root's centre of mass at the shell targets, and the
    walk's (accepted nodes, leaf particles, margin) there."""
    _, e, wt = ref_tree(name, 8)
    pos, mass = inputs(name)
    pts = shell_targets(name).reshape(-1, 3)
    rows = [node_series(pos, mass, e["com"][0], t, KMAX, swap_yz) for t in pts]
    walks = [wt.terms(SHELL_THETA, t)[4:7] for t in pts]
    out = (np.array([r[0] for r in rows], dtype=L), np.array([r[1] for r in rows], dtype=L),
           np.array(walks))
    _frozen(*out)
    return out


def rel_pot(a, b):
    """max |a - b| / |b| with b the long-double side."""
    return float(np.max(np.abs(np.asarray(a, dtype=L) - b) / np.abs(b)))


def rel_acc(a, b):
    d = np.asarray(a, dtype=L) - b
    return float(np.max(np.sqrt((d * d).sum(axis=-1)) / np.sqrt((b * b).sum(axis=-1))))
