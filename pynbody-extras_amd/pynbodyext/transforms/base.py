"""Transform nodes and chains — the part of the reference's
core/calculate/transforms.py the frame transforms need: ``move_all``,
``measure_with`` / ``filter`` / ``with_filter`` (where the parameters are
measured; the downstream snapshot is not narrowed), ``then`` /
``TransformBase.chain`` and :class:`TransformChain`.

The reference applies a transform by rewriting the snapshot's arrays and
reverts it afterwards.  Here a transform never touches the snapshot: a chain
resolves to a :class:`~pynbodyext.frame.Frame`, step by step —

* step k measures its parameters in the frame built by the steps before it,
  under its own measure filter (a calculator parameter runs through the
  calculator layer on a FrameView, so it takes the device routes with the
  frame so far);
* it then extends the frame: a shift of an array not shifted yet, before
  any rotation (and, for positions, before the wrap), sets ``c`` / ``vc``; a
  wrap (transforms/wrap.py) before any rotation sets ``(L, lo)``; the first
  rotation sets ``R``;
* anything else — a second shift of the same array, a shift after a
  rotation, a position shift after the wrap, a second wrap, a wrap after a
  rotation, a second rotation — materialises: ``Frame.apply`` builds a root
  snapshot in the frame so far (numpy, float64) and the chain goes on from
  it with an empty frame.  A sub-snapshot or float32 ``pos`` / ``vel`` are
  materialised before the first step.

Calling a transform on a snapshot returns the snapshot in that frame (a
FrameView, or the materialised snapshot); use ``calculator.transform(t)`` to
evaluate a calculator there.
"""
from __future__ import annotations

import copy

import numpy as np

from ..calculate import CalculatorBase, ExecutionContext, FilterBase, NodeInput
from ..frame import Frame, FrameView, unframe
from ..simcore import SimSnap, SubSnap

__all__ = ["TransformBase", "TransformChain", "chain_transforms"]


def _canonical_source(sim) -> bool:
    """A root snapshot of the snapshot layer whose pos / vel the device
    passes read in place (float64, C order)."""
    if not isinstance(sim, SimSnap) or isinstance(sim, (SubSnap, FrameView)):
        return False
    for key in ("pos", "vel"):
        a = sim._arrays.get(key)
        if a is not None and (a.dtype != np.float64 or not a.flags.c_contiguous):
            return False
    return True


class TransformBase(CalculatorBase):
    """Base of the transform nodes."""

    param_name: str | None = None  # the attribute holding the measured parameter

    def __init__(self, move_all: bool = True):
        # (kept for the reference's signature: a frame covers every particle
        # of the snapshot the calculator is given, whatever it is a view of)
        self.move_all = move_all
        self.measure_filter: FilterBase | None = None

    # -- scoping: where the parameters are measured ------------------------------
    def measure_with(self, filt: FilterBase | None) -> "TransformBase":
        """A copy that measures its parameters on ``filt``."""
        out = copy.copy(self)
        out.measure_filter = filt
        return out

    def with_filter(self, filt: FilterBase) -> "TransformBase":
        """Measure on a filtered view without narrowing the downstream snapshot."""
        return self.measure_with(filt)

    def filter(self, filt: FilterBase) -> "TransformBase":
        return self.measure_with(filt)

    # -- chaining ------------------------------------------------------------------
    @classmethod
    def chain(cls, *transforms: "TransformBase") -> "TransformBase":
        return chain_transforms(*transforms)

    def then(self, transform: "TransformBase") -> "TransformBase":
        return chain_transforms(self, transform)

    def steps(self) -> tuple["TransformBase", ...]:
        return (self,)

    # -- one step --------------------------------------------------------------------
    def measure(self, ctx: ExecutionContext, view):
        """The step's parameter, measured on ``view`` (the snapshot in the
        frame so far) under the measure filter."""
        v = getattr(self, self.param_name)
        if isinstance(v, CalculatorBase):
            node = v if self.measure_filter is None else v.filter(self.measure_filter)
            return ctx.public_value(node, NodeInput(view))
        if callable(v):
            sim = view
            if self.measure_filter is not None:
                sim = view[ctx.raw_value(self.measure_filter, NodeInput(view))]
            return v(sim)
        return v

    def extend(self, frame: Frame, value) -> Frame | None:
        """``frame`` followed by this step with the measured ``value``, or
        None when that is not a canonical frame."""
        raise NotImplementedError

    def measure_in(self, ctx: ExecutionContext, base, frame: Frame):
        """(base, frame, value): the step's parameter measured on ``base`` in
        ``frame``.  A step may hand back a materialised ``base`` with an empty
        frame when it had to measure there (a wrap after a rotation)."""
        view = base if frame.empty else FrameView(base, frame)
        return base, frame, self.measure(ctx, view)

    # -- evaluation --------------------------------------------------------------------
    def framed_sim(self, ctx: ExecutionContext, sim):
        """``sim`` in the frame this transform leads to: ``sim`` itself (an
        empty frame), a FrameView of it, or a materialised snapshot."""
        base, frame = unframe(sim)
        frame = frame if frame is not None else Frame()
        if not _canonical_source(base):
            base, frame = Frame().apply(sim), Frame()
        for step in self.steps():
            base, frame, value = step.measure_in(ctx, base, frame)
            nxt = step.extend(frame, value)
            if nxt is None:  # not canonical: go on from the materialised snapshot
                base = frame.apply(base)
                nxt = step.extend(Frame(), value)
            frame = nxt
        return base if frame.empty else FrameView(base, frame)

    def execute(self, ctx: ExecutionContext, input: NodeInput):
        with ctx.phase(self, "transform"):
            return self.framed_sim(ctx, input.active_sim)


class TransformChain(TransformBase):
    """Transform nodes evaluated in order, each in the frame of those before it."""

    def __init__(self, *transforms: TransformBase):
        if not transforms:
            raise ValueError("At least one transform must be provided.")
        super().__init__()
        flat: list[TransformBase] = []
        for t in transforms:
            if not isinstance(t, TransformBase):
                raise TypeError(f"TransformChain only accepts transform nodes, got {type(t)!r}")
            flat.extend(t.steps())
        self.transforms = tuple(flat)

    def steps(self):
        return self.transforms

    def measure_with(self, filt):
        raise TypeError("a chain has no parameters of its own: set the measure filter on a step")

    def then(self, transform: TransformBase) -> TransformBase:
        return chain_transforms(*self.transforms, transform)

    def __repr__(self):
        return f"TransformChain({', '.join(map(repr, self.transforms))})"


def chain_transforms(*transforms: TransformBase) -> TransformBase:
    return TransformChain(*transforms)
