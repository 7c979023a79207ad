"""AlignVec / AlignAngMomVec — reference pynbodyext/transforms/rotate.py.

The rotation is pynbody's face-on matrix of the measured vector
(simcore.calc_faceon_matrix); it becomes the ``R`` of the frame
(transforms/base.py) instead of a ``Rotation`` of the snapshot's arrays.
"""
from __future__ import annotations

import numpy as np

from ..frame import Frame
from ..properties.generic import AngMomVec
from ..simcore import calc_faceon_matrix
from .base import TransformBase

__all__ = ["AlignAngMomVec", "AlignVec"]


class AlignVec(TransformBase):
    """Align a vector (e.g. the angular momentum) with the z axis.

    vector: array, callable of the snapshot, or calculator.  up: the desired
    direction of +y after the rotation; None picks a safe one from the
    measured vector (``_safe_up``)."""

    dynamic_param_specs = {"vector": None}
    param_name = "vector"

    def __init__(self, vector, up=None, move_all: bool = True):
        super().__init__(move_all=move_all)
        self.vector = vector
        self.up = up

    def instance_signature(self):
        return (self.__class__.__name__, self.up)

    def extend(self, frame: Frame, value):
        vec = np.asarray(value, dtype=np.float64).reshape(3)
        safe_up = self._safe_up(vec, up=None) if self.up is None else self.up
        return frame.with_rotation(calc_faceon_matrix(vec, up=safe_up))

    @staticmethod
    def _safe_up(ang, up=None, parallel_tol: float = 1e-6) -> np.ndarray:
        """A unit 'up' vector that is not (nearly) parallel to ``ang``: the
        preferred ``up`` (default, and for a zero or NaN ``up``: [0, 1, 0]), or
        the coordinate axis least aligned with ``ang`` when the two are
        parallel within ``parallel_tol``."""
        direction = np.asarray(ang, dtype=float)
        length = np.linalg.norm(direction)
        if length == 0 or np.isnan(direction).any():
            raise ValueError(f"Angular momentum vector is zero or NaN {direction}")
        direction = direction / length
        y_axis = np.array([0.0, 1.0, 0.0])
        chosen = y_axis if up is None else np.asarray(up, dtype=float)
        if np.isnan(chosen).any() or np.linalg.norm(chosen) == 0:
            chosen = y_axis
        chosen = chosen / np.linalg.norm(chosen)
        if abs(np.dot(direction, chosen)) <= 1.0 - parallel_tol:
            return chosen
        # (nearly) parallel: the axis with the smallest component of the direction
        return np.eye(3)[np.argmin(np.abs(direction))]

    def __repr__(self):
        return f"AlignVec({self.vector!r}, up={self.up!r})"


AlignAngMomVec = AlignVec(AngMomVec())
"""Aligns the angular momentum vector with the z axis."""
