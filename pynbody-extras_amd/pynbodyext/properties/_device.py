"""Device route of the property calculators (libpbx, csrc/property.hip).

Thin ctypes wrappers of pbx_property_moments(_frame, _region),
pbx_property_shrink_center, pbx_property_enclosed,
pbx_property_virial_radius and pbx_property_wrap_extents (include/pbx.h,
"scalar properties"), and the
conditions under which a property takes them: the source is a root
``SimSnap`` of the snapshot layer — or a FrameView of one, whose frame then
rides along in the pass — whose ``pos`` / ``vel`` / ``mass`` are float64 and
C-contiguous and that stores no user array named ``vcxy`` or ``ke``.
Everything else runs the property's ``calculate`` on the host.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_int64, c_void_p

import numpy as np

from .. import _native as nat
from .. import region as rg
from ..frame import FrameView, unframe
from ..simcore import SimSnap, SubSnap

# group bits and sum layout (pbx.h PBX_PROP_*)
MASS, COM, COV, ANGMOM, KAPPA, KAPPA_MEAN, PATTERN = 1, 2, 4, 8, 16, 32, 64
ALL_GROUPS = 127
NSUMS = 18
POS_GROUPS = COM | ANGMOM | KAPPA | KAPPA_MEAN | PATTERN
VEL_GROUPS = COV | ANGMOM | KAPPA | KAPPA_MEAN | PATTERN
# the enclosed pass (pbx.h PBX_ENCLOSED_* / PBX_VIRIAL_LEVELS)
ENCLOSED_MAX = 31
ENCLOSED_NEXT = 7
ENCLOSED_LEVELS = 5
VIRIAL_LEVELS = 4

_i64p = ctypes.POINTER(c_int64)


def _particle_args(arrays, on_device, n):
    """(pointers, n, keep-alive) of (N,3) / (N,) float64 host arrays or device pointers."""
    if on_device:
        return list(arrays), int(n), ()
    keep, ptrs, count = [], [], None
    for k, a in enumerate(arrays):
        if a is None:
            ptrs.append(None)
            continue
        a = np.ascontiguousarray(np.asarray(a), dtype=np.float64)
        width3 = k < len(arrays) - 1  # (the last one is the mass)
        if (width3 and (a.ndim != 2 or a.shape[1] != 3)) or (not width3 and a.ndim != 1):
            raise ValueError("pos and vel must be (N,3), mass (N,)")
        if count is not None and a.shape[0] != count:
            raise ValueError("pos, vel and mass must have the same length")
        count = a.shape[0]
        keep.append(a)
        ptrs.append(a.ctypes.data_as(c_void_p))
    if count is None:
        count = int(n) if n is not None else 0
    return ptrs, count, tuple(keep)


def _scope_args(sphere, families):
    """(use_sphere, sphere[4], fam, nfam, keep-alive): a filter's device_spec
    as pbx_profile_select takes it."""
    sph = np.zeros(4)
    if sphere is not None:
        cen, radius = sphere
        radius = float(radius)
        sph[:3] = np.asarray(cen, dtype=np.float64).reshape(3)
        sph[3] = radius * radius
    fam = np.zeros(2, dtype=np.int64)
    nfam = 0
    if families is not None:
        fam = np.ascontiguousarray(np.asarray(families, dtype=np.int64).reshape(-1, 2))
        nfam = fam.shape[0]
        if nfam == 0:  # an empty family set keeps nothing
            fam = np.array([[0, 0]], dtype=np.int64)
            nfam = 1
    return int(sphere is not None), sph, fam, nfam


def moments(pos, vel, mass, *, groups: int, sphere=None, families=None, on_device: bool = False,
            n: int | None = None, frame=None, region=None) -> tuple[int, np.ndarray]:
    """(n_kept, sums[18]) of the kept particles in one device pass
    (pbx_property_moments): the count and the sums of the requested groups,
    the others 0.0.  pos / vel / mass: host arrays, or device pointers with
    ``on_device=True`` and ``n``; any of them may be None when no requested
    group (and no sphere) reads it (mass None: unit masses).  frame (a
    pynbodyext.frame.Frame): the pass reads the particles in it, the sphere's
    centre is in its coordinates (pbx_property_moments_frame).  region (a
    list of pynbodyext.region clauses): ANDed with the sphere and the
    families, on the frame's coordinates (pbx_property_moments_region; pos is
    then required)."""
    ptrs, count, keep = _particle_args((pos, vel, mass), on_device, n)
    use_sphere, sph, fam, nfam = _scope_args(sphere, families)
    kept = c_int64(0)
    sums = np.zeros(NSUMS)
    if region:
        framed = frame is not None and not frame.empty
        packed = frame.packed() if framed else None
        nc, kinds, neg, params = rg.packed(region)
        nat.call("pbx_property_moments_region", ptrs[0], ptrs[1], ptrs[2], count, int(on_device),
                 use_sphere, nat.dptr(sph), fam.ctypes.data_as(_i64p), nfam, int(groups),
                 frame.flags if framed else 0, nat.dptr(packed), nc, kinds, neg,
                 nat.dptr(params), byref(kept), nat.dptr(sums))
    elif frame is None or frame.empty:
        nat.call("pbx_property_moments", ptrs[0], ptrs[1], ptrs[2], count, int(on_device),
                 use_sphere, nat.dptr(sph), fam.ctypes.data_as(_i64p), nfam, int(groups),
                 byref(kept), nat.dptr(sums))
    else:
        packed = frame.packed()
        nat.call("pbx_property_moments_frame", ptrs[0], ptrs[1], ptrs[2], count, int(on_device),
                 use_sphere, nat.dptr(sph), fam.ctypes.data_as(_i64p), nfam, int(groups),
                 frame.flags, nat.dptr(packed), byref(kept), nat.dptr(sums))
    del keep
    return kept.value, sums


def shrink_center(pos, mass, *, r0: float, shrink_factor: float = 0.7, min_particles: int = 100,
                  families=None, on_device: bool = False,
                  n: int | None = None) -> tuple[np.ndarray, int, int]:
    """(centre[3], iterations, n_last): the shrinking-sphere centre of the
    particles in the family ranges, the loop of simcore.shrink_sphere_center
    driven by the library over data that stays on the device
    (pbx_property_shrink_center)."""
    ptrs, count, keep = _particle_args((pos, mass), on_device, n)
    _, _, fam, nfam = _scope_args(None, families)
    cen = np.zeros(3)
    it, last = c_int64(0), c_int64(0)
    nat.call("pbx_property_shrink_center", ptrs[0], ptrs[1], count, int(on_device),
             fam.ctypes.data_as(_i64p), nfam, float(r0), float(shrink_factor), int(min_particles),
             nat.dptr(cen), byref(it), byref(last))
    del keep
    return cen, it.value, last.value


def _enclosed_scope(pos, mass, on_device, n, sphere, families, frame, region):
    """The arguments pbx_property_enclosed and pbx_property_virial_radius
    share, in order, and what has to outlive the call."""
    ptrs, count, keep = _particle_args((pos, mass), on_device, n)
    use_sphere, sph, fam, nfam = _scope_args(sphere, families)
    framed = frame is not None and not frame.empty
    fpacked = frame.packed() if framed else None
    nc, kinds, neg, params = rg.packed(region)
    args = (ptrs[0], ptrs[1], count, int(on_device), use_sphere, nat.dptr(sph),
            fam.ctypes.data_as(_i64p), nfam, frame.flags if framed else 0, nat.dptr(fpacked), nc,
            kinds, neg, nat.dptr(params))
    return args, (keep, sph, fam, fpacked, kinds, neg, params)


def enclosed(pos, mass, thresholds=(), *, sphere=None, families=None, on_device: bool = False,
             n: int | None = None, frame=None, region=None,
             extrema: bool = True) -> tuple[int, np.ndarray, np.ndarray, np.ndarray | None]:
    """(n_kept, msum[nt], count[nt], ext[7] or None) of one enclosed pass
    (pbx_property_enclosed): per threshold t the mass and the number of the
    kept particles with ``sqrt((x*x + y*y) + z*z) < t`` (strict), and, with
    ``extrema``, min x, max x, min y, max y, min z, max z, max r of the kept
    particles (NaN when nothing is kept).  At most ENCLOSED_MAX thresholds;
    none: the extrema and the count alone.  Scope arguments as in
    :func:`moments`; mass None: unit masses."""
    t = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    args, alive = _enclosed_scope(pos, mass, on_device, n, sphere, families, frame, region)
    kept = c_int64(0)
    msum = np.zeros(max(t.size, 1))
    count = np.zeros(max(t.size, 1), dtype=np.int64)
    ext = np.zeros(ENCLOSED_NEXT) if extrema else None
    nat.call("pbx_property_enclosed", *args, int(t.size), nat.dptr(t) if t.size else None,
             byref(kept), nat.dptr(msum), count.ctypes.data_as(_i64p), nat.dptr(ext))
    del alive
    return kept.value, msum[:t.size], count[:t.size], ext


def virial_radius(pos, mass, *, target_rho: float, eta: float, niter_max: int = 200,
                  r_max: float | None = None, levels: int = 0, sphere=None, families=None,
                  on_device: bool = False, n: int | None = None, frame=None,
                  region=None) -> tuple[float, int, int, int, bool]:
    """(radius, iterations, passes, n_kept, converged): the bisection of
    simcore.virial_radius driven by the library over data that stays on the
    device (pbx_property_virial_radius), ``levels`` bisection levels decided
    per pass (0: the library's choice, VIRIAL_LEVELS).  r_max None:
    max x - min x of the kept particles."""
    args, alive = _enclosed_scope(pos, mass, on_device, n, sphere, families, frame, region)
    radius = np.zeros(1)
    it, passes, kept, status = c_int64(0), c_int64(0), c_int64(0), ctypes.c_int(0)
    nat.call("pbx_property_virial_radius", *args, float(target_rho), float(eta), int(niter_max),
             int(r_max is not None), 0.0 if r_max is None else float(r_max), int(levels),
             nat.dptr(radius), byref(it), byref(passes), byref(kept), byref(status))
    del alive
    return float(radius[0]), it.value, passes.value, kept.value, status.value == 0


def wrap_extents(pos, boxsize: float, *, frame=None, on_device: bool = False,
                 n: int | None = None) -> np.ndarray:
    """ext[12] of one streaming pass over every particle
    (pbx_property_wrap_extents): per axis min / max of the "center" wrap and
    min / max of the "upper" wrap of the positions in ``frame`` — which may
    hold shifts only; a rotation or a wrap in it is a ValueError.  No
    particles: the identities (+inf, -inf).  The choice per axis is
    pynbodyext.frame.choose_lower."""
    if on_device:
        ptr, count, keep = pos, int(n), None
    else:
        keep = np.ascontiguousarray(np.asarray(pos), dtype=np.float64)
        if keep.ndim != 2 or keep.shape[1] != 3:
            raise ValueError("pos must be (N,3)")
        ptr, count = keep.ctypes.data_as(c_void_p), keep.shape[0]
    framed = frame is not None and not frame.empty
    packed = frame.packed() if framed else None
    ext = np.zeros(12)
    nat.call("pbx_property_wrap_extents", ptr, count, int(on_device),
             frame.flags if framed else 0, nat.dptr(packed), float(boxsize), nat.dptr(ext))
    del keep
    return ext


# -- routing -------------------------------------------------------------------
def snapshot_arrays(source, fields) -> dict | None:
    """The snapshot's arrays of ``fields`` when the device route may read
    them in place, else None (the property then runs on the host)."""
    if not isinstance(source, SimSnap) or isinstance(source, (SubSnap, FrameView)):
        return None
    stored = source._arrays
    if "vcxy" in stored or "ke" in stored:  # a user's own column wins: host route
        return None
    out = {}
    for f in fields:
        a = stored.get(f)
        if a is None or a.dtype != np.float64 or not a.flags.c_contiguous:
            return None
        if a.shape != ((len(source), 3) if f in ("pos", "vel") else (len(source),)):
            return None
        out[f] = a
    return out


def moments_plan(prop, source, spec: dict):
    """Device plan of a property declaring ``device_groups`` and
    ``finish(n_kept, sums, sim)``.  A FrameView source: its base's arrays
    and its frame go to the pass; ``finish`` gets the view."""
    base, frame = unframe(source)
    groups = prop.device_groups
    sphere, families, region = spec.get("sphere"), spec.get("families"), spec.get("region")
    fields = ["mass"] if groups != KAPPA_MEAN else []
    if sphere is not None or region or groups & POS_GROUPS:
        fields.append("pos")
    if groups & VEL_GROUPS:
        fields.append("vel")
    arrs = snapshot_arrays(base, fields)
    if arrs is None:
        return None

    def run():
        n_kept, sums = moments(arrs.get("pos"), arrs.get("vel"), arrs.get("mass"), groups=groups,
                               sphere=sphere, families=families, n=len(source), frame=frame,
                               region=region)
        return prop.finish(n_kept, sums, source)

    return run
