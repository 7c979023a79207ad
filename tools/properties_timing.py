"""Time the property pass on device-resident inputs (profiles/properties/README.md).

    python tools/properties_timing.py [--sizes 1000000,16000000] [--out FILE]

Per size: pbx_property_moments with groups MASS|COM and with all groups, and
one shrinking-sphere solve, each bracketed by the library's own events
(pbx_event_*, on the library stream; a call ends in its stream sync, so the
bracket holds the pass, the reduction and the read-back).  Median of 20
after 3 warm-ups, beside bytes / 6.3 TB/s.  One JSON line per figure.
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
from pynbodyext.properties import _device as pdev  # noqa: E402
from pynbodyext.synthetic import plummer  # noqa: E402

HBM = 6.3e12  # achievable bytes / s (the microarchitecture guide's figure)


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
    ap.add_argument("--sizes", default="1000000,16000000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nat.load()
    nat.set_device(0)
    lines = []
    for n in (int(s) for s in args.sizes.split(",")):
        pos, _ = plummer(n, seed=1002)
        rng = np.random.default_rng(7)
        vel = rng.normal(size=(n, 3))
        mass = rng.uniform(0.5, 1.5, n)
        pos += np.array([0.3, -0.2, 0.1])
        dp, dv, dm = (nat.DeviceArray.from_host(a) for a in (pos, vel, mass))
        for label, groups, nbytes in (("mass|com", pdev.MASS | pdev.COM, 32), ("all", pdev.ALL_GROUPS, 56)):
            med, lo, hi, (kept, _) = timed(lambda g=groups: pdev.moments(
                dp.ptr, dv.ptr, dm.ptr, groups=g, on_device=True, n=n))
            lines.append({"what": "moments", "groups": label, "n": n, "n_kept": kept,
                          "call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi,
                          "bytes": nbytes * n, "bytes_over_6.3TBps_ms": nbytes * n / HBM * 1e3})
        x = pos[:, 0]
        r0 = float((x.max() - x.min()) / 2)
        med, lo, hi, (cen, it, last) = timed(lambda: pdev.shrink_center(
            dp.ptr, dm.ptr, r0=r0, on_device=True, n=n))
        passes = it + 2  # the plain centre of mass, it shrink steps, the pass that stops
        lines.append({"what": "shrink_center", "n": n, "iterations": it, "n_last": last,
                      "passes": passes, "call_ms_median": med, "call_ms_min": lo, "call_ms_max": hi,
                      "bytes": 32 * n * passes,
                      "bytes_over_6.3TBps_ms": 32 * n * passes / HBM * 1e3,
                      "centre": [float(c) for c in cen]})
        for a in (dp, dv, dm):
            a.free()
    text = "\n".join(json.dumps(rec) for rec in lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
