"""Time RadiusAtSurfaceDensity's device steps on device-resident inputs
(profiles/radius_at_density/README.md).

    python tools/radius_at_density_timing.py [--sizes 1000000,16000000] [--out FILE]

Per size: one fused selection of every particle (rxy), then
pbx_profile_cum_build (the stable sort and the one-lane cumulative sum) and
pbx_profile_cum_solve (one launch, one read-back), each bracketed by the
library's own events (pbx_event_*, on the library stream; a call ends in its
stream sync).  Median of 20 after 3 warm-ups.  Beside them the host route
(RadiusAtSurfaceDensity.calculate on a snapshot of the same arrays) by the
host clock, fewer repetitions (it takes seconds).  One JSON line per figure.
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
from pynbodyext.profiles._device import DeviceBins  # noqa: E402
from pynbodyext.properties import RadiusAtSurfaceDensity  # noqa: E402
from pynbodyext.simcore import SimSnap  # noqa: E402
from pynbodyext.synthetic import plummer  # noqa: E402

EPS = 0.01


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


def host_timed(fn, reps, warm=1):
    for _ in range(warm):
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
    for n in (int(s) for s in args.sizes.split(",")):
        pos, _ = plummer(n, seed=1002)
        mass = np.random.default_rng(7).uniform(0.5, 1.5, n) * (100.0 / n)
        # a target the total surface density crosses near the half-mass radius
        rxy = np.sort(np.sqrt(pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]))
        target = round(0.9 * 50.0 / (np.pi * rxy[n // 2] ** 2), 3)
        dp, dm = nat.DeviceArray.from_host(pos), nat.DeviceArray.from_host(mass)
        d = DeviceBins.select(dp.ptr, dm.ptr, on_device=True, n=n, ndim=2)
        assert d.n == n
        med, lo, hi, (r_min, r_max, total) = timed(d.cum_build)
        lines.append({"what": "cum_build", "n": n, "call_ms_median": med, "call_ms_min": lo,
                      "call_ms_max": hi, "r_min": r_min, "r_max": r_max, "total": total})
        grid = np.linspace(max(r_min, EPS), r_max, 256)
        for mode in ("total", "shell"):
            med, lo, hi, (radius, info) = timed(
                lambda m=mode: d.cum_solve(target, grid, mode=m, eps=EPS))
            lines.append({"what": "cum_solve", "mode": mode, "n": n, "target": target,
                          "call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi,
                          "radius": radius, "info": [int(v) for v in info]})
        d.close()
        dp.free()
        dm.free()
        sim = SimSnap({"pos": pos, "mass": mass})
        prop = RadiusAtSurfaceDensity(target, mode="total", eps=EPS)
        reps = 5 if n <= 2_000_000 else 3
        med, lo, hi, value = host_timed(lambda: prop(sim, backend="host"), reps)
        lines.append({"what": "host_calculate", "mode": "total", "n": n, "target": target,
                      "reps": reps, "call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi,
                      "radius": float(value)})
        t0 = time.perf_counter()
        res = prop.run(sim, perf_time=True)  # the public device route, host arrays staged
        lines.append({"what": "public_device_route", "mode": "total", "n": n, "target": target,
                      "call_ms": (time.perf_counter() - t0) * 1e3,
                      "device_phase_ms": res.perf["RadiusAtSurfaceDensity.device"] * 1e3,
                      "radius": float(res.value)})
    text = "\n".join(json.dumps(rec) for rec in lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
