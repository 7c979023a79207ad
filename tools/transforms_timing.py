"""Time the passes that carry a frame (profiles/transforms/README.md).

    python tools/transforms_timing.py [--sizes 1000000,16000000] [--out FILE]

Per size, for KappaRot (the property pass, group KAPPA) and for the equaln
128-bin profile with vphi (selection + binning + mass sums, then the fused
kinematic sums of vphi):

* ``device / full frame`` and ``device / empty frame``: the same pass on
  device-resident arrays with a full frame (shift, boost, rotation) and
  without one — their ratio is what the frame costs a pass that streams
  56 B (64 B) per particle;
* ``host / fused frame``: the pass on host arrays with the frame (staging
  included), what ``calculator.transform(...)`` runs;
* ``host / materialised``: ``Frame.pos`` / ``Frame.vel`` in numpy, then the
  frame-less pass on the rewritten host arrays — what a user had to do.

Each figure is the median of 20 calls after 3 warm-ups, bracketed by the
library's own events (pbx_event_*, on the library stream); a call ends in a
stream sync, so a bracket is a call time (host work between the events
included), not a kernel time.  One JSON line per figure.
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
from pynbodyext.profiles._device import SRC_NONE, SRC_W, DeviceBins  # noqa: E402
from pynbodyext.properties import _device as pdev  # noqa: E402
from pynbodyext.synthetic import plummer  # noqa: E402

SPHERE = ((0.0, 0.0, 0.0), 8.0)
STATS = [(SRC_W, SRC_NONE, 1 << 3)]


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = nat.Event(), nat.Event()
        e0.record()
        fn()
        e1.record()
        nat.call("pbx_stream_synchronize")
        ms.append(e0.elapsed_ms(e1))
    return statistics.median(ms), min(ms), max(ms)


def euler(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    rz = np.array([[ca, -sa, 0.0], [sa, ca, 0.0], [0.0, 0.0, 1.0]])
    ry = np.array([[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cc, -sc], [0.0, sc, cc]])
    return rz @ ry @ rx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,16000000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nat.load()
    nat.set_device(0)
    frame = Frame(c=[0.3, -0.2, 0.1], vc=[0.05, 0.4, -0.25], R=euler(0.4, -0.9, 1.7))
    lines = []

    def record(what, route, n, t):
        lines.append({"what": what, "route": route, "n": n, "call_ms_median": t[0],
                      "call_ms_min": t[1], "call_ms_max": t[2]})
        print(json.dumps(lines[-1]), flush=True)

    for n in (int(s) for s in args.sizes.split(",")):
        pos, _ = plummer(n, seed=1002)
        pos += frame.c
        rng = np.random.default_rng(7)
        vel = rng.normal(size=(n, 3)) + frame.vc
        mass = rng.uniform(0.5, 1.5, n)
        dp, dv, dm = (nat.DeviceArray.from_host(a) for a in (pos, vel, mass))
        h = DeviceBins()

        def kappa(p, v, m, fr, on_device):
            return pdev.moments(p, v, m, groups=pdev.KAPPA, sphere=SPHERE, frame=fr,
                                on_device=on_device, n=n)

        def profile(p, v, m, fr, on_device):
            h.set_frame(fr)
            DeviceBins.radial_equaln(p, m, nbins=128, sphere=SPHERE, stats=STATS, on_device=on_device,
                                     n=n, into=h)
            h.set_kinematics(p, v, on_device=on_device, n=n)
            return h.kinematic_moments(["vphi"], SRC_W, 0b11)

        for what, fn in (("kappa_rot", kappa), ("profile_equaln128_vphi", profile)):
            record(what, "device / full frame", n,
                   timed(lambda: fn(dp.ptr, dv.ptr, dm.ptr, frame, True)))
            record(what, "device / empty frame", n,
                   timed(lambda: fn(dp.ptr, dv.ptr, dm.ptr, None, True)))
            record(what, "host / fused frame", n, timed(lambda: fn(pos, vel, mass, frame, False)))
            record(what, "host / materialised", n,
                   timed(lambda: fn(frame.pos(pos), frame.vel(vel), mass, None, False)))
        h.close()
        for a in (dp, dv, dm):
            a.free()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(rec) for rec in lines) + "\n")


if __name__ == "__main__":
    main()
