"""WrapBox and the frame's wrap on the host route (no device is touched).

The fixture tests/golden/wrapbox.npz holds the reference's own wrapped
positions (tests/golden/make_golden_wrap.py): 5 box sizes x 6 position sets x
3 conventions, with planted rows at 0.0, -0.0, +-L, +-L/2 and one set per box
whose |k| exceeds an int8.  Everything here is compared bit for bit.
"""
import logging
import warnings
from pathlib import Path

import numpy as np
import pytest

import pynbodyext.transforms as transforms
from pynbodyext.calculate import ConstantProperty
from pynbodyext.frame import Frame, FrameView, choose_lower, wrap_axis, wrap_extents
from pynbodyext.simcore import SimSnap
from pynbodyext.transforms import AlignVec, ShiftPosTo, ShiftVelTo
from pynbodyext.transforms.wrap import WrapBox

HOST = {"backend": "host"}
UNITS = {"pos": "kpc", "vel": "km s**-1", "mass": "Msol"}
GOLD = np.load(Path(__file__).resolve().parent / "golden" / "wrapbox.npz")
BOXES = GOLD["boxes"]
CONVENTIONS = [str(c) for c in GOLD["conventions"]]
NSETS = int(GOLD["nsets"])
NO_BOX = "wrap: no boxsize specified and snapshot has no 'boxsize' property; skipping wrap"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def snap(pos, boxsize=None, vel=None):
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    n = len(pos)
    arrays = {"pos": pos, "vel": np.zeros((n, 3)) if vel is None else vel, "mass": np.ones(n)}
    props = {} if boxsize is None else {"boxsize": boxsize}
    return SimSnap(arrays, families={"dm": slice(0, n)}, units_map=UNITS, properties=props)


def lower_of(conv, L, pos):
    if conv == "minirange":
        return choose_lower(wrap_extents(pos, L), L)
    return np.full(3, -0.5 * L if conv == "center" else 0.0)


# ------------------------------------------------------------------ fixture
@pytest.mark.parametrize("b", range(len(BOXES)))
def test_fixture_through_frame(b):
    L = float(BOXES[b])
    zeros = 0
    for s in range(NSETS):
        pos = GOLD[f"pos/{b}/{s}"]
        assert pos.shape[0] <= 4096
        for conv in CONVENTIONS:
            ref = GOLD[f"ref/{b}/{s}/{conv}"]
            got = Frame(wrap=(L, lower_of(conv, L, pos))).pos(pos)
            assert np.array_equal(bits(got), bits(ref)), (L, s, conv)
            zeros += np.count_nonzero(bits(ref) == bits(-0.0))
    assert zeros > 0  # (the planted -0.0 rows are in the fixture and come back as -0.0)


@pytest.mark.parametrize("b", range(len(BOXES)))
def test_fixture_through_wrapbox(b):
    L = float(BOXES[b])
    for s in range(NSETS):
        pos = GOLD[f"pos/{b}/{s}"]
        for conv in CONVENTIONS:
            sim = snap(pos.copy(), L)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                view = WrapBox(convention=conv)(sim, **HOST)
            assert isinstance(view, FrameView) and view._frame_base is sim
            assert np.array_equal(bits(view["pos"]), bits(GOLD[f"ref/{b}/{s}/{conv}"])), (L, s, conv)
            assert np.array_equal(bits(sim["pos"]), bits(pos))  # (the snapshot is untouched)


def test_plus_zero_is_needed():
    """Without the "+ 0.0" a -0.0 coordinate would come back as +0.0."""
    v = np.array([-0.0])
    assert np.signbit(wrap_axis(v, 3.0, 0.0))[0]
    k = np.floor((v - 0.0) / 3.0)
    assert not np.signbit(v - k * 3.0)[0]


# --------------------------------------------------------------- frame rules
def test_frame_rules_and_packing():
    L, lo = 7.5, np.array([-3.75, 0.0, -3.75])
    c, vc = np.array([1.0, 2.0, 3.0]), np.array([4.0, 5.0, 6.0])
    R = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    plain = Frame(c, vc, R)
    assert plain.flags == 7 and plain.packed().shape == (15,)
    assert np.array_equal(plain.packed(), np.concatenate([c, vc, R.reshape(9)]))
    assert Frame().packed().shape == (15,) and Frame().empty

    w = Frame().with_wrap(L, lo)
    assert w.flags == 16 and not w.empty and w.packed().shape == (19,)
    assert np.array_equal(w.packed(), np.concatenate([np.zeros(15), [L], lo]))
    assert w.with_wrap(L, lo) is None            # a second wrap
    assert w.with_pos_shift(c) is None           # a position shift after the wrap
    assert Frame(R=R).with_wrap(L, lo) is None   # a wrap after the rotation
    assert Frame(R=R).with_pos_shift(c) is None  # (as before)
    full = Frame(c).with_wrap(L, lo).with_vel_shift(vc).with_rotation(R)
    assert full.flags == (1 | 2 | 4 | 16)
    assert np.array_equal(full.packed(), np.concatenate([c, vc, R.reshape(9), [L], lo]))
    assert Frame(c).with_wrap(L, lo).flags == (16 | 1)
    assert full.with_rotation(R) is None and full.with_vel_shift(vc) is None
    assert "wrap=" in repr(full)
    for bad_L in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="box size"):
            Frame(wrap=(bad_L, np.zeros(3)))
    with pytest.raises(ValueError, match="lo of a wrap"):
        Frame(wrap=(L, np.array([0.0, 1.0, 0.0])))


def test_frame_order_and_velocities():
    """shift, then wrap, then rotation; velocities are never wrapped."""
    rng = np.random.default_rng(5)
    L = 9.3
    pos, vel = rng.uniform(0, L, (200, 3)), rng.normal(scale=50.0, size=(200, 3))
    c, lo = np.array([9.0, 0.2, 4.0]), np.array([-0.5 * L, -0.5 * L, 0.0])
    R = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    f = Frame(c, None, R, (L, lo))
    by_hand = np.stack([wrap_axis(pos[:, k] - c[k], L, lo[k]) for k in range(3)], axis=1)
    by_hand = Frame(R=R).pos(by_hand)
    assert np.array_equal(bits(f.pos(pos)), bits(by_hand))
    assert np.array_equal(bits(f.vel(vel)), bits(Frame(R=R).vel(vel)))
    sim = snap(pos, L, vel)
    out = f.apply(sim)
    assert np.array_equal(bits(out["pos"]), bits(by_hand)) and out.properties["boxsize"] == L
    assert np.array_equal(bits(FrameView(sim, f)["pos"]), bits(by_hand))


# ------------------------------------------------------------------- WrapBox
def test_constructor_and_signature():
    with pytest.raises(ValueError) as e:
        WrapBox(convention="lower")
    assert str(e.value) == "Unknown wrapping convention, must be 'center', 'upper' or 'minirange'"
    w = WrapBox()
    assert (w.boxsize, w.convention, w.move_all) == (None, "minirange", True)
    assert WrapBox.dynamic_param_specs == {"boxsize": "pos"}
    assert WrapBox(3.0, "upper").instance_signature() == ("WrapBox", 3.0, "upper")


@pytest.mark.parametrize("boxsize, text", [
    (None, NO_BOX),
    (0.0, "wrap: boxsize must be positive, got 0.0; skipping wrap"),
    (-2.5, "wrap: boxsize must be positive, got -2.5; skipping wrap"),
])
def test_warnings_leave_the_frame_unchanged(boxsize, text, caplog):
    pos = np.random.default_rng(1).uniform(-5, 5, (50, 3))
    sim = snap(pos)
    c = np.array([1.0, 2.0, 3.0])
    with caplog.at_level(logging.WARNING, logger="pynext"):
        with pytest.warns(UserWarning) as rec:
            alone = WrapBox(boxsize)(sim, **HOST)
        assert [str(w.message) for w in rec] == [text]
        assert [r.getMessage() for r in caplog.records if r.name == "pynext"] == [text]
        assert alone is sim
        with pytest.warns(UserWarning):
            view = ShiftPosTo(c).then(WrapBox(boxsize))(sim, **HOST)
    assert view._frame.flags == 1 and view._frame.wrap is None
    assert np.array_equal(bits(view["pos"]), bits(Frame(c).pos(pos)))


def test_skipped_wrap_after_a_rotation_does_not_materialise():
    """No box size, or L <= 0, behind a rotation: the frame is left as it was,
    a view of the same snapshot; with a box size the same chain materialises."""
    pos = np.random.default_rng(3).uniform(-5, 5, (50, 3))
    vec = np.array([0.3, -0.5, 0.8])
    for sim, boxsize in ((snap(pos), None), (snap(pos, 4.0), 0.0), (snap(pos, 4.0), -1.0)):
        with pytest.warns(UserWarning, match="skipping wrap"):
            view = AlignVec(vec).then(WrapBox(boxsize))(sim, **HOST)
        assert isinstance(view, FrameView) and view._frame_base is sim
        assert view._frame.flags == 4 and view._frame.wrap is None
        with pytest.warns(UserWarning, match="skipping wrap"):
            twice = WrapBox(3.0, "upper").then(WrapBox(boxsize))(sim, **HOST)
        assert twice._frame_base is sim and twice._frame.flags == 16
    sim = snap(pos, 4.0)
    late = AlignVec(vec).then(WrapBox())(sim, **HOST)
    assert late._frame_base is not sim and late._frame.flags == 16
    empty = snap(np.zeros((0, 3)), 4.0)
    assert AlignVec(vec).then(WrapBox())(empty, **HOST)._frame_base is empty


def test_a_callable_with_a_ratio_attribute_is_called():
    class Box:
        ratio = 2.0  # (not a unit: a user's callable that happens to have the name)

        def __call__(self, sim):
            return 6.0

    sim = snap(np.random.default_rng(4).uniform(-9, 9, (20, 3)), 10.0)
    assert WrapBox(Box(), "upper")(sim, **HOST)._frame.wrap[0] == 6.0


def test_explicit_boxsize_beats_the_property():
    pos = np.random.default_rng(2).uniform(-20, 20, (300, 3))
    sim = snap(pos, 10.0)
    assert WrapBox(convention="upper")(sim, **HOST)._frame.wrap[0] == 10.0
    for given, L in ((4.0, 4.0), ("4 kpc", 4.0), ("0.004 Mpc", 4.0), (lambda s: 0.5 * len(s), 150.0),
                     (ConstantProperty(4.0), 4.0)):
        view = WrapBox(given, convention="upper")(sim, **HOST)
        assert view._frame.wrap[0] == pytest.approx(L, rel=1e-12), given
        L = view._frame.wrap[0]
        assert np.array_equal(bits(view["pos"]), bits(Frame(wrap=(L, np.zeros(3))).pos(pos)))
    assert WrapBox(4.0, convention="upper")(sim, **HOST)._frame.wrap[0] == 4.0  # (exactly)
    # a unit string in the snapshot's property converts too
    assert WrapBox(convention="center")(snap(pos, "0.01 Mpc"), **HOST)._frame.wrap[0] == \
        pytest.approx(10.0, rel=1e-12)


def test_minirange_choices():
    L = 8.0
    # x: both ranges equal (one particle): the tie goes to center
    # y: a cloud across the face at 0 / L: center is tighter
    # z: a cloud around L/2: upper is tighter
    pos = np.array([[1.0, 0.5, 3.5], [1.0, 7.5, 4.5], [1.0, 7.75, 4.25]])
    ext = wrap_extents(pos, L)
    assert ext[1] - ext[0] == ext[3] - ext[2] == 0.0
    assert np.array_equal(choose_lower(ext, L), [-4.0, -4.0, 0.0])
    view = WrapBox()(snap(pos, L), **HOST)
    assert np.array_equal(view._frame.wrap[1], [-4.0, -4.0, 0.0])
    assert np.array_equal(view["pos"], [[1.0, 0.5, 3.5], [1.0, -0.5, 4.5], [1.0, -0.25, 4.25]])
    # a NaN coordinate: that axis's ranges are NaN, the comparison is false: upper
    pos2 = np.array([[0.5, 0.5, 0.5], [7.5, 7.5, np.nan], [7.75, 7.75, 7.75]])
    ext2 = wrap_extents(pos2, L)
    assert np.isnan(ext2[8:12]).all() and not np.isnan(ext2[:8]).any()
    view2 = WrapBox()(snap(pos2, L), **HOST)
    assert np.array_equal(view2._frame.wrap[1], [-4.0, -4.0, 0.0])
    assert np.isnan(view2["pos"][1, 2]) and view2["pos"][2, 2] == 7.75 and view2["pos"][2, 1] == -0.25


def test_empty_snapshot():
    empty = np.zeros((0, 3))
    assert np.array_equal(wrap_extents(empty, 3.0), np.tile([np.inf, -np.inf], 6))
    sim = snap(empty, 3.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert WrapBox()(sim, **HOST) is sim  # (the reference's empty-axis branch: no wrap)
        view = WrapBox(convention="center")(sim, **HOST)
    assert view["pos"].shape == (0, 3)


# --------------------------------------------------------------------- chains
def test_chains():
    rng = np.random.default_rng(9)
    L = 25.0 / 0.7
    c = np.array([L - 0.3, 0.2, 0.5 * L])
    pos = np.mod(c + rng.normal(scale=1.5, size=(2000, 3)), L)
    vel = rng.normal(scale=100.0, size=(2000, 3))
    sim = snap(pos.copy(), L, vel.copy())
    vec = np.array([0.3, -0.5, 0.8])

    view = ShiftPosTo(c).then(WrapBox())(sim, **HOST)
    assert isinstance(view, FrameView) and view._frame_base is sim
    assert view._frame.flags == (1 | 16)
    assert np.array_equal(view._frame.wrap[1], np.full(3, -0.5 * L))  # a halo: center everywhere
    assert np.array_equal(bits(sim["pos"]), bits(pos))
    shifted = Frame(c).pos(pos)
    wrapped = Frame(wrap=(L, np.full(3, -0.5 * L))).pos(shifted)
    assert np.array_equal(bits(view["pos"]), bits(wrapped))
    assert np.abs(wrapped).max() < 10.0 < np.abs(shifted).max()  # (the halo is whole again)

    view3 = ShiftPosTo(c).then(WrapBox()).then(AlignVec(vec))(sim, **HOST)
    assert isinstance(view3, FrameView) and view3._frame_base is sim
    assert view3._frame.flags == (1 | 16 | 4)
    R = view3._frame.R
    assert np.array_equal(bits(view3["pos"]), bits(Frame(R=R).pos(wrapped)))
    assert np.array_equal(bits(view3["vel"]), bits(Frame(R=R).vel(vel)))

    view4 = ShiftVelTo(np.array([1.0, 2.0, 3.0])).then(WrapBox(None, "upper"))(sim, **HOST)
    assert view4._frame.flags == (2 | 16) and view4._frame_base is sim

    # a wrap after the rotation: materialised, equal to the host statement
    late = AlignVec(vec).then(WrapBox())(sim, **HOST)
    assert late._frame_base is not sim and late._frame.flags == 16
    rotated = Frame(R=R).pos(pos)
    lo = choose_lower(wrap_extents(rotated, L), L)
    assert np.array_equal(bits(late["pos"]), bits(Frame(wrap=(L, lo)).pos(rotated)))
    assert np.array_equal(bits(late["vel"]), bits(Frame(R=R).vel(vel)))
    assert np.array_equal(bits(sim["pos"]), bits(pos))

    # a second wrap and a shift after a wrap materialise too
    twice = WrapBox(convention="upper").then(WrapBox(convention="center"))(sim, **HOST)
    once = Frame(wrap=(L, np.zeros(3))).pos(pos)
    assert np.array_equal(bits(twice["pos"]), bits(Frame(wrap=(L, np.full(3, -0.5 * L))).pos(once)))
    after = WrapBox(convention="upper").then(ShiftPosTo(c))(sim, **HOST)
    assert after._frame_base is not sim and after._frame.flags == 1
    assert np.array_equal(bits(after["pos"]), bits(Frame(c).pos(once)))


def test_exports():
    import pynbodyext.transforms.wrap as wrap_module

    assert wrap_module.__all__ == ["WrapBox"] and wrap_module.WrapBox is WrapBox
    assert "WrapBox" not in transforms.__all__
    assert not hasattr(transforms, "WrapBox") and "__getattr__" not in vars(transforms)
