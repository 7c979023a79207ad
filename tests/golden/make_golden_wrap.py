#!/usr/bin/env python3
"""Generate the WrapBox fixture from the REFERENCE's own code.

Run where a checkout of the reference is at hand (never on the GPU box, not
collected by pytest):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wrap.py REFERENCE_ROOT

It loads REFERENCE_ROOT/pynbodyext/transforms/wrap.py by file path.  The
names that module imports are provided as minimal stand-ins
(pynbody.transformation.Transformation, pynbody.units.UnitBase,
pynbody.array.SimArray, pynbody.snapshot.SimSnap, pynbodyext.calculate's
TransformBase and pynbodyext.log.logger), and a snapshot stand-in hands out
the columns of a plain (N,3) array as ``sim["x"]`` ... with
``ancestor.properties["boxsize"]``.  WrapTransformation._apply_to_snapshot
then rewrites that array in place.  Nothing from the reference is copied into
the repository: tests/golden/wrapbox.npz holds the input positions (160 rows
per set), the box size and convention of each case and the reference's
wrapped positions, with the numpy version used.

The matrix: 5 box sizes x 6 position sets x 3 conventions = 90 cases.  Sets
0-2 are tight clouds (sigma 0.02 L) and sets 3-4 wide ones (0.4 L) around a
centre in [-L, 2L); set 5 is a wide cloud moved by 5 L and scaled by 40, so
that |k| > 127 and the reference promotes the dtype of its integer k.  Every
set carries the planted rows 0.0, -0.0, L, -L, L/2, -L/2, nextafter(L/2, 0)
in x and y and their negatives in z.

The script is the gatekeeper of the definition (pynbodyext.frame.wrap_axis /
choose_lower): a case whose bits the definition does not reproduce is an
error here, never a skipped test.
"""
from __future__ import annotations

import importlib.util
import logging
import sys
import types
import warnings
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
ROOT = OUT.parent.parent
sys.path.insert(0, str(ROOT / "pynbody-extras_amd"))

BOXES = (1.0, 0.3, 25.0 / 0.7, 100.0, 7.123456789)
NSETS = 6
NROWS = 160
CONVENTIONS = ("center", "upper", "minirange")


# ---------------------------------------------------------------- stand-ins
def load_reference(ref_root: Path):
    class Transformation:
        def __init__(self, f, description=None):
            self.sim = f

    class TransformBase:
        def __class_getitem__(cls, item):
            return cls

        def __init__(self, move_all=True):
            pass

    mods = {name: types.ModuleType(name) for name in (
        "pynbody", "pynbody.transformation", "pynbody.units", "pynbody.array", "pynbody.snapshot",
        "pynbodyext", "pynbodyext.calculate", "pynbodyext.log")}
    mods["pynbody.transformation"].Transformation = Transformation
    mods["pynbody.units"].UnitBase = type("UnitBase", (), {})
    mods["pynbody.array"].SimArray = type("SimArray", (np.ndarray,), {})
    mods["pynbody.snapshot"].SimSnap = type("SimSnap", (), {})
    mods["pynbody"].transformation = mods["pynbody.transformation"]
    mods["pynbody"].units = mods["pynbody.units"]
    mods["pynbodyext"].__path__ = []
    mods["pynbodyext.calculate"].TransformBase = TransformBase
    mods["pynbodyext.log"].logger = logging.getLogger("make_golden_wrap.reference")
    saved = {name: sys.modules.get(name) for name in mods}
    sys.modules.update(mods)
    try:
        spec = importlib.util.spec_from_file_location(
            "_reference_wrap", ref_root / "pynbodyext" / "transforms" / "wrap.py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:  # (the package's own modules are imported below)
        for name, old in saved.items():
            if old is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = old
    return mod.WrapTransformation


class Snap:
    """``sim["x"]`` is a writable column of ``pos``; its own ancestor."""

    def __init__(self, pos, boxsize):
        self.pos = pos
        self.properties = {"boxsize": boxsize}
        self.ancestor = self

    def __getitem__(self, key):
        return self.pos[:, "xyz".index(key)]


# ---------------------------------------------------------------- inputs
def position_set(rng, L, s):
    cen = rng.uniform(-L, 2 * L, 3)
    pos = cen + rng.normal(size=(NROWS, 3)) * L * (0.02 if s < 3 else 0.4)
    if s == 5:  # centre in [160 L, 280 L): every k is beyond an int8
        pos = (pos + 5.0 * L) * 40.0
    edge = np.array([0.0, -0.0, L, -L, 0.5 * L, -0.5 * L, np.nextafter(0.5 * L, 0)])
    pos[:7, 0] = edge
    pos[:7, 1] = edge
    pos[:7, 2] = -edge
    return pos


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    wrap_cls = load_reference(Path(sys.argv[1]))
    from pynbodyext.frame import Frame, choose_lower, wrap_extents

    rng = np.random.default_rng(16)
    out = {"numpy_version": np.array(np.__version__), "boxes": np.array(BOXES),
           "conventions": np.array(CONVENTIONS), "nsets": np.array(NSETS)}
    promoted = 0
    minus_zero = 0
    for b, L in enumerate(BOXES):
        for s in range(NSETS):
            pos = position_set(rng, L, s)
            out[f"pos/{b}/{s}"] = pos
            for conv in CONVENTIONS:
                ref = pos.copy()
                t = wrap_cls(Snap(ref, L), convention=conv)
                with warnings.catch_warnings(record=True) as rec:
                    warnings.simplefilter("always")
                    t._apply_to_snapshot(t.sim)
                promoted += any("auto-promote" in str(w.message) for w in rec)
                # the definition, through the frame the package builds
                if conv == "minirange":
                    lo = choose_lower(wrap_extents(pos, L), L)
                else:
                    lo = np.full(3, -0.5 * L if conv == "center" else 0.0)
                mine = Frame(wrap=(L, lo)).pos(pos)
                if not np.array_equal(bits(mine), bits(ref)):
                    bad = np.argwhere(bits(mine) != bits(ref))
                    raise SystemExit(f"L={L!r} set {s} {conv}: the definition differs from the "
                                     f"reference at {bad[:5].tolist()}")
                minus_zero += int(np.count_nonzero(bits(ref) == bits(-0.0)))
                out[f"ref/{b}/{s}/{conv}"] = ref
                if conv == "minirange":
                    out[f"lo/{b}/{s}"] = lo
    assert promoted >= len(BOXES) * len(CONVENTIONS), promoted  # (set 5 of every box)
    assert minus_zero > 0  # (the planted -0.0 rows come back as -0.0)
    np.savez_compressed(OUT / "wrapbox.npz", **out)
    size = (OUT / "wrapbox.npz").stat().st_size
    assert size < 1 << 20, size
    print(f"wrote wrapbox.npz: {len(BOXES) * NSETS * len(CONVENTIONS)} cases, {size} bytes, "
          f"{promoted} with a promoted k dtype, {minus_zero} values of -0.0")


if __name__ == "__main__":
    main()
