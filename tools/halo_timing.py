"""Time the enclosed pass and the virial-radius driver (profiles/halo/README.md).

    python tools/halo_timing.py [--sizes 1000000,16000000] [--out FILE]

Per size, on a Plummer halo with non-uniform masses, with the arrays resident
on the device and again with host arrays (staged by every call):

* the yardstick: pbx_property_moments with PBX_PROP_MASS behind a Sphere that
  keeps every particle (the same 32 bytes per particle);
* pbx_property_enclosed at nt = 0 (extrema only), 1, 3, 7, 15 and
  PBX_ENCLOSED_MAX, without extrema where nt > 0 (what the driver launches);
* pbx_property_virial_radius, the whole call, for L = 1 .. PBX_ENCLOSED_LEVELS;
* numpy's VirialRadius.calculate on a snapshot of the same arrays, by the
  host clock.

Device calls are bracketed by the library's own events (pbx_event_*, on the
library stream; a call ends in its stream sync, so a bracket holds the
staging, the passes, the reductions and the read-backs).  Median of 20 after
3 warm-ups (of 5 after 1 with host arrays), beside bytes / 6.3 TB/s.  One JSON
line per figure.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pynbody-extras_amd"))

from pynbodyext import _native as nat  # noqa: E402
from pynbodyext import simcore  # noqa: E402
from pynbodyext.properties import VirialRadius  # noqa: E402
from pynbodyext.properties import _device as pdev  # noqa: E402
from pynbodyext.synthetic import plummer_chunked  # noqa: E402

HBM = 6.3e12  # achievable bytes / s (the microarchitecture guide's figure)
UNITS = {"pos": "kpc", "vel": "km s**-1", "mass": "Msol"}
PROPERTIES = {"h": 0.7, "omegaM0": 0.3, "omegaL0": 0.7, "z": 0.5}
OVERDENSITY = 200.0


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = nat.Event(), nat.Event()
        e0.record()
        out = fn()
        e1.record()
        nat.call("pbx_stream_synchronize")
        ms.append(e0.elapsed_ms(e1))
    return statistics.median(ms), min(ms), max(ms), out


def host_timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,16000000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nat.load()
    nat.set_device(0)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for n in (int(s) for s in args.sizes.split(",")):
        pos, m = plummer_chunked(n, seed=1002)
        pos *= 10.0
        mass = m * 1.0e12 * np.random.default_rng(7).uniform(0.5, 1.5, n)
        sim = simcore.SimSnap({"pos": pos, "mass": mass}, units_map=UNITS, properties=PROPERTIES)
        target = simcore.virial_target_density(sim, OVERDENSITY)
        radii = np.quantile(np.asarray(sim["r"]), np.linspace(0.03, 0.97, pdev.ENCLOSED_MAX))
        x = pos[:, 0]
        r_all = 4.0 * float(np.abs(pos).max())  # a Sphere that keeps every particle
        dp, dm = nat.DeviceArray.from_host(pos), nat.DeviceArray.from_host(mass)
        for where, (p, w), kw, reps, warm in (
                ("device", (dp.ptr, dm.ptr), {"on_device": True, "n": n}, 20, 3),
                ("host", (pos, mass), {}, 5, 1)):
            base = {"n": n, "arrays": where, "bytes": 32 * n,
                    "bytes_over_6.3TBps_ms": 32 * n / HBM * 1e3}
            med, lo, hi, (kept, _) = timed(lambda: pdev.moments(
                p, None, w, groups=pdev.MASS, sphere=((0.0, 0.0, 0.0), r_all), **kw), reps, warm)
            assert kept == n
            yard = med
            emit({"what": "moments_mass_sphere", **base, "call_ms_median": med, "call_ms_min": lo,
                  "call_ms_max": hi})
            for nt in (0, 1, 3, 7, 15, pdev.ENCLOSED_MAX):
                med, lo, hi, out = timed(lambda nt=nt: pdev.enclosed(
                    p, w, radii[:nt], extrema=(nt == 0), **kw), reps, warm)
                assert out[0] == n
                emit({"what": "enclosed", "nt": nt, "extrema": nt == 0, **base,
                      "call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi,
                      "ratio_to_moments_mass_sphere": med / yard})
            for levels in range(1, pdev.ENCLOSED_LEVELS + 1):
                med, lo, hi, (radius, it, passes, kept, ok) = timed(lambda L=levels: pdev.virial_radius(
                    p, w, target_rho=target, eta=1.0e-3 * target, levels=L, **kw), reps, warm)
                assert ok and kept == n
                emit({"what": "virial_radius", "levels": levels, **base, "radius": radius,
                      "iterations": it, "passes": passes, "call_ms_median": med,
                      "call_ms_min": lo, "call_ms_max": hi,
                      "bytes": 32 * n * passes, "bytes_over_6.3TBps_ms": 32 * n * passes / HBM * 1e3})
        prop = VirialRadius(OVERDENSITY)
        med, lo, hi, value = host_timed(lambda: prop(sim, backend="host"), 5 if n <= 2_000_000 else 3)
        emit({"what": "numpy_calculate", "n": n, "radius": value, "call_ms_median": med,
              "call_ms_min": lo, "call_ms_max": hi, "x_extent": float(x.max() - x.min())})
        med, lo, hi, value = host_timed(lambda: prop(sim), 3)
        emit({"what": "public_device_route", "n": n, "radius": value, "call_ms_median": med,
              "call_ms_min": lo, "call_ms_max": hi})
        dp.free()
        dm.free()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(rec) for rec in lines) + "\n")


if __name__ == "__main__":
    main()
