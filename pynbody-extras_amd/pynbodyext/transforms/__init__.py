"""Coordinate transformations: centre a snapshot, put it at rest, align a
vector with z — reference pynbodyext/transforms (``WrapBox`` is not
provided: periodic wrapping is not an affine frame and needs pynbody's box
properties).

Transforms never rewrite the snapshot.  A chain resolves to a frame of 15
numbers (pynbodyext.frame) that rides along in the device passes::

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
