"""WrapBox — reference pynbodyext/transforms/wrap.py.

The name, the signature, the conventions and the warning / error texts are
the reference's; the wrap becomes the ``(L, lo[3])`` of the frame
(pynbodyext.frame, transforms/base.py), applied between the position shift
and the rotation, instead of an in-place rewrite of ``pos``::

    halo = ShiftPosTo(centre).then(WrapBox())          # a halo across a box face
    prof = RadialProfileBuilder(...).transform(halo)

"center" wraps every axis into ``[-L/2, L/2)``, "upper" into ``[0, L)``;
"minirange" (the default) chooses between the two per axis, whichever leaves
the smaller coordinate range over all particles (the tie goes to center, a
NaN coordinate sends its axis to upper).  That choice needs the extents of
both candidate wraps: one streaming pass on the device
(pbx_property_wrap_extents) when the snapshot is one the device passes read in
place, numpy on the view otherwise — the same 12 numbers either way
(pynbodyext.frame.wrap_extents / choose_lower).

Deviation from the reference: an explicit ``boxsize`` is
honoured, as the reference's docstring says; its code reads only
``sim.properties["boxsize"]``.

This module is the public home of ``WrapBox``, as in the reference:
``from pynbodyext.transforms.wrap import WrapBox``.  It is not re-exported
from ``pynbodyext.transforms`` yet.
"""
from __future__ import annotations

import warnings

import numpy as np

from .._pyn import units as _units
from ..calculate import CalculatorBase, ExecutionContext, resolve_value_in_units
from ..frame import Frame, FrameView, choose_lower, unframe, wrap_extents
from ..log import logger
from .base import TransformBase, _canonical_source

__all__ = ["WrapBox"]

_NO_BOX = "wrap: no boxsize specified and snapshot has no 'boxsize' property; skipping wrap"


def _warn(text: str) -> None:
    warnings.warn(text, stacklevel=3)
    logger.warning(text)


class WrapBox(TransformBase):
    """Wrap the positions into a periodic box.

    boxsize: the box size — a number, a unit string or unit object (converted
    to the snapshot's position units), a callable of the snapshot or a
    calculator; None reads ``sim.properties["boxsize"]``.  convention:
    "center", "upper" or "minirange".  Velocities are not touched.

    A measure filter (``.filter(...)`` / ``.measure_with(...)``) scopes a
    calculator or callable ``boxsize`` only: the extents "minirange" chooses
    from are always taken over every particle of the snapshot, as in the
    reference."""

    dynamic_param_specs = {"boxsize": "pos"}
    param_name = "boxsize"

    def __init__(self, boxsize=None, convention="minirange", move_all: bool = True):
        if convention not in ("center", "upper", "minirange"):
            raise ValueError(
                "Unknown wrapping convention, must be 'center', 'upper' or 'minirange'")
        super().__init__(move_all=move_all)
        self.boxsize = boxsize
        self.convention = convention

    def instance_signature(self):
        return (self.__class__.__name__, self.boxsize, self.convention)

    # -- one step ------------------------------------------------------------------
    def _resolve_boxsize(self, ctx: ExecutionContext, view) -> float | None:
        v = self.boxsize
        if v is None:
            try:
                v = view.properties["boxsize"]
            except (AttributeError, KeyError):
                return None
        elif isinstance(v, CalculatorBase) or (
                callable(v) and not isinstance(v, getattr(_units, "UnitBase", ()))):
            v = super().measure(ctx, view)
        v = resolve_value_in_units(v, view, "pos")
        return float(np.asarray(v, dtype=np.float64).reshape(()))

    def _extents(self, ctx: ExecutionContext, view, L: float) -> np.ndarray:
        """The 12 extents of every particle of ``view`` in the frame so far."""
        base, frame = unframe(view)
        pos = base._arrays.get("pos") if _canonical_source(base) else None
        if ctx.on_host or pos is None:
            return wrap_extents(view["pos"], L)
        from ..properties import _device as pdev

        return pdev.wrap_extents(pos, L, frame=frame)

    def measure_in(self, ctx: ExecutionContext, base, frame: Frame):
        """(base, frame, (L, lo[3]) or None).  The box size is resolved in the
        frame so far; only when a wrap will be applied and does not fit that
        frame (a wrap is set already, or a rotation) is the snapshot
        materialised — before the extents are taken, so that they come from
        the new root, which the device pass can read."""
        view = base if frame.empty else FrameView(base, frame)
        L = self._resolve_boxsize(ctx, view)
        if L is None:
            _warn(_NO_BOX)
            return base, frame, None
        if L <= 0:
            _warn(f"wrap: boxsize must be positive, got {L}; skipping wrap")
            return base, frame, None
        if self.convention == "minirange" and len(view) == 0:
            return base, frame, None  # (the reference's empty-axis branch: no wrap)
        if frame.wrap is not None or frame.R is not None:
            base, frame = frame.apply(base), Frame()
            view = base
        if self.convention == "center":
            lo = np.full(3, -0.5 * L)
        elif self.convention == "upper":
            lo = np.zeros(3)
        else:
            lo = choose_lower(self._extents(ctx, view, L), L)
        return base, frame, (L, lo)

    def extend(self, frame: Frame, value):
        if value is None:
            return frame
        return frame.with_wrap(*value)

    def __repr__(self):
        return f"WrapBox({self.boxsize!r}, convention={self.convention!r})"
