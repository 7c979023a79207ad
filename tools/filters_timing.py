"""Time the passes that carry a region (profiles/filters/README.md).

    python tools/filters_timing.py [--tree DIR] [--sizes 16000000] [--out FILE]

Per size, on device-resident arrays, behind ``Sphere(8)`` about the origin:

* ``property``: the property pass, groups MASS | COM (32 B per particle);
* ``selection``: ``pbx_profile_radial_equaln``, 128 equaln bins with mass sums
  (the lazy selection and everything downstream of it),

each ``sphere only`` and with a ``5-clause region`` ANDed in (a disc, a
negated sphere, a cuboid, an x band and an rxy band, chosen wide enough to
keep most of what the Sphere keeps, so that both routes do the same work
downstream of the predicate).  ``--tree DIR`` imports the package of another
checkout (the parent commit's, built there): a tree without
``pynbodyext.region`` reports the ``sphere only`` routes alone.

Each figure is the median of 20 calls after 3 warm-ups, bracketed by the
library's own events (pbx_event_*, on the library stream); a call ends in a
stream sync, so a bracket is a call time, not a kernel time.  One JSON line
per figure.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SPHERE = ((0.0, 0.0, 0.0), 8.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=str(ROOT))
    ap.add_argument("--sizes", default="16000000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.tree).resolve() / "pynbody-extras_amd"))

    from pynbodyext import _native as nat
    from pynbodyext.profiles._device import SRC_NONE, SRC_W, DeviceBins
    from pynbodyext.properties import _device as pdev
    from pynbodyext.synthetic import plummer

    try:
        from pynbodyext import region as rg
    except ImportError:
        rg = None
    label = args.label or ("this" if rg is not None else "parent")
    nat.load()
    nat.set_device(0)
    stats = [(SRC_W, SRC_NONE, 1 << 3)]
    region = None
    if rg is not None:
        region = [rg.disc_clause((0.0, 0.0, 0.0), 7.5, 7.0), rg.sphere_clause((0.0, 0.0, 0.0), 0.05, True),
                  rg.cuboid_clause(-7.0, -7.0, -7.0, 7.0, 7.0, 7.0), rg.band_clause("x", -6.5, None),
                  rg.band_clause("rxy", 0.01, 7.4)]

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

    lines = []

    def record(what, route, n, kept, t):
        lines.append({"build": label, "what": what, "route": route, "n": n, "kept": kept,
                      "call_ms_median": t[0], "call_ms_min": t[1], "call_ms_max": t[2]})
        print(json.dumps(lines[-1]), flush=True)

    for n in (int(s) for s in args.sizes.split(",")):
        pos, _ = plummer(n, seed=1002)
        mass = np.random.default_rng(7).uniform(0.5, 1.5, n)
        dp, dm = nat.DeviceArray.from_host(pos), nat.DeviceArray.from_host(mass)
        h = DeviceBins()
        for route, kw in (("sphere only", {}), ("5-clause region", {"region": region})):
            if kw and region is None:
                continue

            def prop():
                return pdev.moments(dp.ptr, None, dm.ptr, groups=pdev.MASS | pdev.COM, sphere=SPHERE,
                                    on_device=True, n=n, **kw)

            def sel():
                return DeviceBins.radial_equaln(dp.ptr, dm.ptr, nbins=128, sphere=SPHERE, stats=stats,
                                                on_device=True, n=n, into=h, **kw)

            record("property", route, n, int(prop()[0]), timed(prop))
            sel()
            record("selection", route, n, int(h.n), timed(sel))
        h.close()
        dp.free()
        dm.free()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(rec) + "\n" for rec in lines))


if __name__ == "__main__":
    main()
