"""Time the frame's wrap and the wrap-extents pass (profiles/wrap/README.md).

    python tools/wrap_timing.py [--sizes 16000000] [--out FILE]

Per size, on a Plummer halo around a point near a box corner reduced into
[0, L), with the arrays resident on the device:

* pbx_property_moments with PBX_PROP_MASS | PBX_PROP_COM behind a Sphere that
  keeps every particle: without a frame, with a shift, with a shift and a
  wrap (32 bytes per particle each);
* pbx_property_wrap_extents without and with a shift (24 bytes per particle).

Device calls are bracketed by the library's own events (pbx_event_*, on the
library stream; a call ends in its stream sync, so a bracket is a call time:
the pass, its reduction and the read-back).  Median of 20 after 3 warm-ups,
beside bytes / 6.3 TB/s.  One JSON line per figure.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pynbody-extras_amd"))

from pynbodyext import _native as nat  # noqa: E402
from pynbodyext.frame import Frame  # noqa: E402
from pynbodyext.properties import _device as pdev  # noqa: E402
from pynbodyext.synthetic import plummer_chunked  # noqa: E402

HBM = 6.3e12  # achievable bytes / s (the microarchitecture guide's figure)
BOX = 25.0 / 0.7


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16000000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nat.load()
    nat.set_device(0)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    centre = np.array([BOX - 0.4, 0.3, BOX - 0.2])
    lo = np.full(3, -0.5 * BOX)
    for n in (int(s) for s in args.sizes.split(",")):
        off, m = plummer_chunked(n, seed=1002)
        pos = np.mod(centre + off, BOX)
        mass = m * np.random.default_rng(7).uniform(0.5, 1.5, n)
        dp, dm = nat.DeviceArray.from_host(pos), nat.DeviceArray.from_host(mass)
        on = {"on_device": True, "n": n}
        everything = ((0.0, 0.0, 0.0), 4.0 * BOX)
        frames = {"none": None, "shift": Frame(centre), "shift+wrap": Frame(centre, wrap=(BOX, lo))}
        yard = None
        for name, fr in frames.items():
            med, mn, mx, (kept, _) = timed(lambda fr=fr: pdev.moments(
                dp.ptr, None, dm.ptr, groups=pdev.MASS | pdev.COM, sphere=everything, frame=fr, **on))
            assert kept == n
            yard = med if yard is None else yard
            emit({"what": "moments_mass_com_sphere", "frame": name, "n": n, "bytes": 32 * n,
                  "bytes_over_6.3TBps_ms": 32 * n / HBM * 1e3, "call_ms_median": med,
                  "call_ms_min": mn, "call_ms_max": mx, "ratio_to_no_frame": med / yard})
        for name, fr in (("none", None), ("shift", Frame(centre))):
            med, mn, mx, ext = timed(lambda fr=fr: pdev.wrap_extents(dp.ptr, BOX, frame=fr, **on))
            assert np.isfinite(ext).all()
            emit({"what": "wrap_extents", "frame": name, "n": n, "bytes": 24 * n,
                  "bytes_over_6.3TBps_ms": 24 * n / HBM * 1e3, "call_ms_median": med,
                  "call_ms_min": mn, "call_ms_max": mx})
        dp.free()
        dm.free()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(rec) for rec in lines) + "\n")


if __name__ == "__main__":
    main()
