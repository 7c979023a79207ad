"""Time the three routes to a profile's velocity anisotropy inputs (the
per-bin mean and rms of vr, vtheta and vphi) on one GPU.

  a  the host-column route (what the code offered before the device derived
     the fields): numpy builds the three N-long columns, they are stored in
     the snapshot, and pro[f]["rms"] runs for each (a host gather of the kept
     rows, one upload and two per-bin passes per field);
  b  the three fields through the SRC_KIN source selector, one generic
     per-bin pass each (the field written to and re-read from HBM);
  c  one fused kinematic_moments call.

Every route is timed behind Sphere(10) & FamilyFilter("dm"), equaln 128,
weight mass, on a Plummer sphere with seeded standard-normal velocities
(pynbodyext.synthetic gives none).  The profile (selection and bins) is built
outside the timed window; a timed window ends in a device synchronise (every
call returns host results).  Route a also runs on a build that predates the
device fields: point --pkg at that tree's package directory, and routes b and
c are skipped there.

usage: python tools/kinematics_ab.py [--sizes 1000000,16000000] [--reps 7]
           [--routes a,b,c] [--pkg DIR] [--out FILE.json]
Prints one JSON line per size and writes them to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ("vr", "vtheta", "vphi")


def columns(pos, vel):
    """The three columns as a user computes them with numpy (pynbody's
    expressions; vtheta in the algebraic form)."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    vx, vy, vz = vel[:, 0], vel[:, 1], vel[:, 2]
    with np.errstate(all="ignore"):
        rxy = np.sqrt(x * x + y * y)
        r = np.sqrt((x * x + y * y) + z * z)
        s = x * vx + y * vy
        return {"vr": (s + z * vz) / r, "vtheta": (z * (s / rxy) - rxy * vz) / r,
                "vphi": (x * vy - y * vx) / rxy}


def med(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,16000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--routes", default="a,b,c")
    ap.add_argument("--pkg", default=str(ROOT / "pynbody-extras_amd"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.pkg)

    from pynbodyext import _native as nat
    from pynbodyext.filters import FamilyFilter, Sphere
    from pynbodyext.profiles import RadialProfileBuilder
    from pynbodyext.profiles import _device as dv
    from pynbodyext.simcore import SimSnap
    from pynbodyext.synthetic import family_slices, plummer_chunked

    nat.load()
    nat.set_device(0)
    routes = [r for r in args.routes.split(",") if r]
    has_kin = hasattr(dv, "SRC_KIN")
    if not has_kin:
        routes = [r for r in routes if r == "a"]
    cols = 1 << 0 | 1 << 1 | 1 << 2  # Σw, Σf·w, Σf²·w: the weighted mean and rms
    builder = RadialProfileBuilder(ndim=3, weight="mass", bins_type="equaln", nbins=128).filter(
        Sphere(10.0) & FamilyFilter("dm"))
    lines = []
    for n in (int(s) for s in args.sizes.split(",")):
        pos, mass = plummer_chunked(n, seed=1002)
        vel = np.random.default_rng(2002).standard_normal((n, 3))
        fams = family_slices(n)
        rec = {"tool": "kinematics_ab", "label": args.label, "n": n,
               "pkg": os.path.relpath(args.pkg, ROOT), "device": nat.device_name(), "routes": {}}
        res = {}
        for rep in range(args.reps + 1):  # (rep 0 warms every route up)
            t = {}
            if "a" in routes:
                sim = SimSnap({"pos": pos, "vel": vel, "mass": mass}, families=fams)
                t0 = time.perf_counter()
                for f, c in columns(pos, vel).items():
                    sim[f] = c
                t1 = time.perf_counter()
                pro = builder(sim)
                t2 = time.perf_counter()
                out_a = [np.asarray(pro[f]["rms"]) for f in FIELDS]
                t3 = time.perf_counter()
                t["a_columns"], t["a_statistics"] = t1 - t0, t3 - t2
                t["a_total"] = t["a_columns"] + t["a_statistics"]
                res["a"] = out_a
                rec["kept"] = len(pro.sim)
            if "b" in routes or "c" in routes:
                sim = SimSnap({"pos": pos, "vel": vel, "mass": mass}, families=fams)
                pro = builder(sim)
                dev = pro.bins._device
                t0 = time.perf_counter()
                dev.set_kinematics(pos, vel)
                t["register"] = time.perf_counter() - t0
                rec["kept"] = len(pro.sim)
                if "b" in routes:
                    t0 = time.perf_counter()
                    mb = [dev.moments(dv.SRC_KIN(f), dv.SRC_W, cols) for f in FIELDS]
                    t["b_src_kin"] = time.perf_counter() - t0
                    res["b"] = [np.sqrt(m[:, 2] / m[:, 0]) for m in mb]
                if "c" in routes:
                    t0 = time.perf_counter()
                    mc = dev.kinematic_moments(FIELDS, dv.SRC_W, cols)
                    t["c_fused"] = time.perf_counter() - t0
                    res["c"] = [np.sqrt(m[:, 2] / m[:, 0]) for m in mc]
                # the user-level call on a fresh profile: registration + the fused pass
                pro2 = builder(sim)
                t0 = time.perf_counter()
                np.asarray(pro2["beta"])
                t["beta_end_to_end"] = time.perf_counter() - t0
            if rep:
                for k, v in t.items():
                    rec["routes"].setdefault(k, []).append(v)
        # the routes compute the same numbers
        keys = sorted(res)
        for k in keys[1:]:
            for u, v in zip(res[keys[0]], res[k]):
                np.testing.assert_allclose(u, v, rtol=1e-12)
        rec["agree_rtol_1e-12"] = keys
        rec["routes"] = {k: med(v) for k, v in rec["routes"].items()}
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
