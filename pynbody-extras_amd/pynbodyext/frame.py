"""The frame a calculator reads a snapshot in.

A :class:`Frame` is what a chain of transforms (pynbodyext.transforms)
amounts to while it stays canonical: an optional position shift ``c``, an
optional velocity shift ``vc``, an optional periodic wrap of the positions
(box size ``L``, lower bound ``lo`` per axis) and an optional rotation
``R``, applied per particle in float64 in exactly this order (include/pbx.h,
pbx_profile_set_frame)::

    dx = x - c0;  dy = y - c1;  dz = z - c2                 (only if c is set)
    k  = floor((dx - lo0) / L) + 0.0;  dx = dx - k * L      (only if the wrap is
    ... the same for dy, dz with lo1, lo2                    set; positions only)
    x' = (R00*dx + R01*dy) + R02*dz;  y' = (R10*dx + R11*dy) + R12*dz
    z' = (R20*dx + R21*dy) + R22*dz                         (only if R is set)

and the same for ``v`` with ``vc`` (a velocity is never wrapped).  A step
that is not set is skipped, not run with zeros or the identity (0 * inf would
turn an infinity into NaN).  The wrap takes a coordinate into ``[lo, lo + L)``
with ``lo = -0.5 * L`` (the reference's "center") or ``0.0`` ("upper"): the
division is IEEE division, and the ``+ 0.0`` turns a ``-0.0`` from ``floor``
into ``+0.0`` so that ``-0.0`` stays ``-0.0``, which is what the reference's
integer ``k`` gives (:func:`wrap_axis`).
:func:`apply_half` is this statement in numpy: it is the definition the
device kernels (csrc/frame.h) reproduce bit for bit, and what every host
route evaluates.  pynbody's own ``Rotation`` goes through ``np.dot``, whose
summation order is the BLAS library's; parity with it is not pinned
(DESIGN.md §5).

The 15 numbers (19 with a wrap) ride along in the device passes (the property pass, the
profile handle's selection and kinematic fields), so nothing rewrites
``pos`` / ``vel``.  Host consumers get a :class:`FrameView`: the snapshot
with ``pos``, ``vel``, their columns and the fields derived from them in the
frame, computed on demand; every other array passes through.
"""
from __future__ import annotations

from collections.abc import Mapping

import numpy as np

from .simcore import SimSnap, SubSnap

__all__ = ["Frame", "FrameView", "apply_half", "unframe", "wrap_axis", "wrap_extents",
           "choose_lower"]

FRAME_POS, FRAME_VEL, FRAME_ROT, FRAME_WRAP = 1, 2, 4, 16  # include/pbx.h PBX_FRAME_*


def wrap_axis(v, L: float, lo: float) -> np.ndarray:
    """One coordinate column wrapped into ``[lo, lo + L)``: the definition of
    the frame's wrap step (float64, IEEE division, no FMA)."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        k = np.floor((v - lo) / L) + 0.0  # "+ 0.0": a -0.0 from floor becomes +0.0
        return v - k * L


def wrap_extents(pos, L: float) -> np.ndarray:
    """The 12 numbers a "minirange" wrap chooses from (include/pbx.h,
    pbx_property_wrap_extents), from (N,3) positions already in the frame so
    far: per axis min / max of the "center" wrap, then min / max of the
    "upper" wrap, numpy's min / max (a NaN wins); no particles: the
    identities."""
    pos = np.asarray(pos, dtype=np.float64)
    out = np.tile([np.inf, -np.inf], 6)
    if pos.shape[0] == 0:
        return out
    for a in range(3):
        wc, wu = wrap_axis(pos[:, a], L, -0.5 * L), wrap_axis(pos[:, a], L, 0.0)
        out[4 * a:4 * a + 4] = wc.min(), wc.max(), wu.min(), wu.max()
    return out


def choose_lower(ext, L: float) -> np.ndarray:
    """lo[3] of a "minirange" wrap from its 12 extents: per axis "center"
    (``-0.5 * L``) when its range is <= the "upper" range, else "upper"
    (``0.0``).  The tie goes to center; a NaN range makes the comparison false
    and chooses upper, as in the reference."""
    ext = np.asarray(ext, dtype=np.float64).reshape(3, 4)
    with np.errstate(all="ignore"):
        range_c, range_u = ext[:, 1] - ext[:, 0], ext[:, 3] - ext[:, 2]
        return np.where(range_c <= range_u, -0.5 * L, 0.0)


def apply_half(a, shift, rot, wrap=None) -> np.ndarray:
    """(N,3) array ``a`` shifted by ``shift`` (or None), wrapped by ``wrap`` =
    ``(L, lo[3])`` (or None) and rotated by the row-major ``rot`` (or None),
    in float64, in the module's order.  Always a new float64 array."""
    a = np.asarray(a, dtype=np.float64)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    with np.errstate(all="ignore"):
        if shift is not None:
            x, y, z = x - shift[0], y - shift[1], z - shift[2]
        if wrap is not None:
            L, lo = wrap
            x, y, z = wrap_axis(x, L, lo[0]), wrap_axis(y, L, lo[1]), wrap_axis(z, L, lo[2])
        if rot is not None:
            r = rot
            x, y, z = ((r[0, 0] * x + r[0, 1] * y) + r[0, 2] * z,
                       (r[1, 0] * x + r[1, 1] * y) + r[1, 2] * z,
                       (r[2, 0] * x + r[2, 1] * y) + r[2, 2] * z)
    out = np.empty(a.shape, dtype=np.float64)
    out[:, 0], out[:, 1], out[:, 2] = x, y, z
    return out


def _vec3(v, what):
    v = np.array(v, dtype=np.float64).reshape(-1)
    if v.shape != (3,):
        raise ValueError(f"{what} must have 3 components")
    return v


class Frame:
    """Position shift ``c``, velocity shift ``vc``, rotation ``R``, wrap
    ``(L, lo[3])`` (each None or set).  Immutable: the ``with_*`` methods
    return the extended frame, or None when the step does not fit the
    canonical order (a second shift of the same array, a shift after the
    rotation, a second rotation, a position shift after the wrap, a wrap
    after a wrap or a rotation) and the caller has to materialise
    (:meth:`apply`)."""

    __slots__ = ("c", "vc", "R", "wrap")

    def __init__(self, c=None, vc=None, R=None, wrap=None):
        self.c = None if c is None else _vec3(c, "c")
        self.vc = None if vc is None else _vec3(vc, "vc")
        if R is not None:
            R = np.array(R, dtype=np.float64)
            if R.shape != (3, 3):
                raise ValueError("R must be 3 x 3")
        self.R = R
        if wrap is not None:
            L, lo = float(wrap[0]), _vec3(wrap[1], "lo")
            if not (np.isfinite(L) and L > 0):
                raise ValueError(f"the box size of a wrap must be finite and positive, got {L}")
            if not all(v == 0.0 or v == -0.5 * L for v in lo):
                raise ValueError(f"lo of a wrap must be -0.5 * L or 0.0 per axis, got {lo.tolist()}")
            wrap = (L, lo)
        self.wrap = wrap

    @property
    def empty(self) -> bool:
        return self.c is None and self.vc is None and self.R is None and self.wrap is None

    def with_pos_shift(self, c) -> "Frame | None":
        if self.c is not None or self.R is not None or self.wrap is not None:
            return None
        return Frame(c, self.vc, None)

    def with_vel_shift(self, vc) -> "Frame | None":
        if self.vc is not None or self.R is not None:
            return None
        return Frame(self.c, vc, None, self.wrap)

    def with_rotation(self, R) -> "Frame | None":
        if self.R is not None:
            return None
        return Frame(self.c, self.vc, R, self.wrap)

    def with_wrap(self, L, lo) -> "Frame | None":
        if self.wrap is not None or self.R is not None:
            return None
        return Frame(self.c, self.vc, None, (L, lo))

    # -- what the device takes --------------------------------------------------
    @property
    def flags(self) -> int:
        return ((FRAME_POS if self.c is not None else 0) | (FRAME_VEL if self.vc is not None else 0)
                | (FRAME_ROT if self.R is not None else 0)
                | (FRAME_WRAP if self.wrap is not None else 0))

    def packed(self) -> np.ndarray:
        """frame[15] = {c[3], vc[3], R[9]} (unset parts 0: their flag is off);
        with a wrap frame[19] = {c[3], vc[3], R[9], L, lo[3]}."""
        out = np.zeros(15 if self.wrap is None else 19)
        if self.c is not None:
            out[0:3] = self.c
        if self.vc is not None:
            out[3:6] = self.vc
        if self.R is not None:
            out[6:15] = self.R.reshape(9)
        if self.wrap is not None:
            out[15], out[16:19] = self.wrap
        return out

    # -- the numpy restatement --------------------------------------------------
    def pos(self, pos) -> np.ndarray:
        return apply_half(pos, self.c, self.R, self.wrap)

    def vel(self, vel) -> np.ndarray:
        return apply_half(vel, self.vc, self.R)

    def apply(self, sim) -> SimSnap:
        """Materialise: a root snapshot with the same particles, arrays,
        families and units as ``sim`` whose ``pos`` / ``vel`` are float64 and
        in this frame."""
        arrays, units_map = {}, {}
        for k in sim.keys():
            a = np.asarray(sim[k])
            if k == "pos":
                a = self.pos(a)
            elif k == "vel":
                a = self.vel(a)
            arrays[k] = a
            units_map[k] = sim._unit_of(k)
        families = {}
        for f in sim.ancestor._family_slice:
            sl = sim._get_family_slice(f)
            if isinstance(sl, slice):  # (a view in no increasing order has no ranges)
                families[f.name] = slice(*sl.indices(len(sim))[:2])
        return SimSnap(arrays, families=families, units_map=units_map,
                       properties=getattr(sim, "properties", None))

    def __repr__(self):
        parts = [f"{n}={getattr(self, n).tolist()}" for n in ("c", "vc", "R")
                 if getattr(self, n) is not None]
        if self.wrap is not None:
            parts.append(f"wrap=({self.wrap[0]}, {self.wrap[1].tolist()})")
        return f"Frame({', '.join(parts)})"


class _PassThrough(Mapping):
    """A view's stored arrays: the base's, without ``pos`` and ``vel``, read
    only — ``view[key] = ...`` raises instead of writing into the snapshot."""

    _OWN = ("pos", "vel")

    def __init__(self, arrays: dict):
        self._a = arrays

    def __getitem__(self, key):
        if key in self._OWN:
            raise KeyError(key)
        return self._a[key]

    def __setitem__(self, key, value):
        raise TypeError(f"a frame view is read-only ({key!r}): pos / vel are derived from the "
                        "snapshot and every other array is the snapshot's own; write the snapshot")

    def __iter__(self):
        return (k for k in self._a if k not in self._OWN)

    def __len__(self):
        return sum(1 for _ in self)


class FrameView(SimSnap):
    """The root snapshot ``base`` seen in ``frame`` — never a copy of it.

    ``pos`` and ``vel`` (hence x, vx, ..., r, rxy, the kinematic fields, vcxy,
    ke) are the frame's, computed from the base's arrays with the numpy
    restatement the first time one is read and kept for the view's lifetime;
    every other array is the base's own.  The device routes never read them:
    they take the base's arrays and the frame (:func:`unframe`)."""

    def __init__(self, base: SimSnap, frame: Frame):
        if isinstance(base, (SubSnap, FrameView)) or not isinstance(base, SimSnap):
            raise TypeError("a frame view wraps a root snapshot")
        self._frame_base = base
        self._frame = frame
        self._n = len(base)
        self._arrays = _PassThrough(base._arrays)
        self._units = base._units
        self._family_slice = base._family_slice
        self._derived = {}

    def keys(self):
        return self._frame_base.keys()

    @property
    def properties(self) -> dict:
        return self._frame_base.properties

    def _array(self, key: str) -> np.ndarray:
        if key in ("pos", "vel"):
            val = self._derived.get(key)
            if val is None:
                raw = self._frame_base._arrays[key]  # (KeyError: the snapshot has none)
                val = self._frame.pos(raw) if key == "pos" else self._frame.vel(raw)
                self._derived[key] = val
            return val
        return super()._array(key)

    def __repr__(self):
        return f"<FrameView {self._frame!r} of {self._frame_base!r}>"


def unframe(sim):
    """(snapshot, frame): a frame view's base and frame; anything else with
    frame None."""
    if isinstance(sim, FrameView):
        return sim._frame_base, sim._frame
    return sim, None
