"""ShiftPosTo / ShiftVelTo — reference pynbodyext/transforms/shift.py.

Names, signatures and error texts are the reference's; the shift becomes the
``c`` / ``vc`` of the frame (transforms/base.py) instead of a
``GenericTranslation`` of the snapshot's arrays.
"""
from __future__ import annotations

import numpy as np

from .._pyn import SimArray
from ..frame import Frame
from ..properties import CenPos, CenVel
from .base import TransformBase

__all__ = ["ShiftPosTo", "ShiftVelTo"]


def _as_parameter(mode, named: dict, expected: str):
    """(parameter, description) of a shift: a name from ``named`` becomes its
    calculator; a callable or an array is taken as given.  The error texts
    are the reference's."""
    if isinstance(mode, str):
        if mode not in named:
            raise ValueError(f"Invalid mode: {mode}. Expected {expected}.")
        return named[mode](mode), mode
    if callable(mode) or isinstance(mode, (np.ndarray, SimArray)):
        return mode, "given"
    raise ValueError(f"Invalid mode type: {type(mode)}. Expected str, callable, or array.")


class _Shift(TransformBase):
    param_name = "mode"

    def instance_signature(self):
        return (self.__class__.__name__, )

    def __repr__(self):
        return f"{type(self).__name__}({self.description!r})"


class ShiftPosTo(_Shift):
    """Centre the positions on ``mode``: "ssc" / "com" (CenPos), an array, a
    callable of the snapshot or a calculator ("pot" / "hyb" raise as CenPos
    does)."""

    dynamic_param_specs = {"mode": "pos"}
    _NAMED = {name: (lambda m: CenPos(mode=m)) for name in ("ssc", "com", "pot", "hyb")}

    def __init__(self, mode="ssc", move_all: bool = True):
        super().__init__(move_all=move_all)
        self.mode, self.description = _as_parameter(
            mode, self._NAMED, "one of ['ssc', 'com', 'pot', 'hyb']")

    def extend(self, frame: Frame, value):
        return frame.with_pos_shift(np.asarray(value, dtype=np.float64))


class ShiftVelTo(_Shift):
    """Put the velocities at rest with ``mode``: "com" (CenVel), an array, a
    callable of the snapshot or a calculator."""

    dynamic_param_specs = {"mode": "vel"}
    _NAMED = {"com": lambda m: CenVel(mode=m)}

    def __init__(self, mode="com", move_all: bool = True):
        super().__init__(move_all=move_all)
        self.mode, self.description = _as_parameter(mode, self._NAMED, "'com'")

    def extend(self, frame: Frame, value):
        return frame.with_vel_shift(np.asarray(value, dtype=np.float64))
