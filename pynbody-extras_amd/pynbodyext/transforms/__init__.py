"""Coordinate transformations: centre a snapshot, put it at rest, align a
vector with z — reference pynbodyext/transforms.  ``WrapBox`` (the periodic
wrap into the box, between the shift and the rotation) lives in
``pynbodyext.transforms.wrap``, the module the reference defines it in, and
is imported from there: this package does not re-export it yet (DESIGN.md
§7).

Transforms never rewrite the snapshot.  A chain resolves to a frame of 15
numbers, 19 with a wrap (pynbodyext.frame), that rides along in the device
passes::

    krot = KappaRot().filter(Sphere(30.) & FamilyFilter("star")).transform(
        ShiftPosTo("ssc")
        .then(ShiftVelTo("com").filter(Sphere(0.5 * re) & FamilyFilter("star")))
        .then(AlignVec(AngMomVec().filter(Sphere(2 * re) & FamilyFilter("star")))))
"""
from ..frame import Frame, FrameView
from .base import TransformBase, TransformChain, chain_transforms
from .rotate import AlignAngMomVec, AlignVec
from .shift import ShiftPosTo, ShiftVelTo

__all__ = ["AlignVec", "AlignAngMomVec", "ShiftPosTo", "ShiftVelTo", "TransformBase",
           "TransformChain", "chain_transforms", "Frame", "FrameView"]
