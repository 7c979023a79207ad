"""Time ShardedDirect.solve (HIP events on the library stream) for equal and
for jittered masses: the uniform-mass and the general instantiation of
csrc/direct_sym.hip's pair kernel on the same positions.

    python tools/direct_sym_paths.py [--n 1000000] [--steps 5] [--warmup 1]

One JSON line per mass set: per-step ms, median, and the path counters'
increase (null with a library that predates pbx_direct_sym_path_stats, such
as an A/B build named by PBX_AB_LIBRARY).  With GRAVITY_TIMING=1 the library
prints the stream time of the mass check and its read-back to stderr.
"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pynbody-extras_amd"))

from pynbodyext import _native as nat  # noqa: E402
from pynbodyext.parallel import ShardedDirect  # noqa: E402
from pynbodyext.synthetic import plummer  # noqa: E402


def path_stats():
    u, g = ctypes.c_int64(), ctypes.c_int64()
    try:
        nat.call("pbx_direct_sym_path_stats", ctypes.byref(u), ctypes.byref(g))
    except AttributeError:
        return None
    return u.value, g.value


def time_solve(pos, mass, steps, warmup):
    s = ShardedDirect(None, len(pos), pos, mass)
    for _ in range(warmup):
        s.step()
    nat.synchronize()
    before = path_stats()
    ms = []
    for _ in range(steps):
        s.gather_sources()
        e0, e1 = nat.Event(), nat.Event()
        e0.record()
        s.solve()
        e1.record()
        nat.synchronize()
        ms.append(e0.elapsed_ms(e1))
    after = path_stats()
    launches = None if before is None else [after[0] - before[0], after[1] - before[1]]
    return ms, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1002)
    a = ap.parse_args()
    nat.load()
    nat.set_device(0)
    pos, mass = plummer(a.n, seed=a.seed)
    jitter = mass * np.random.default_rng(a.seed).uniform(0.5, 1.5, a.n)
    for name, m in (("uniform", mass), ("jittered", jitter)):
        ms, launches = time_solve(pos, m, a.steps, a.warmup)
        print(json.dumps({"masses": name, "n": a.n, "mode": "precise" if nat.get_precise() else "fast",
                          "solve_ms": [round(x, 3) for x in ms],
                          "median_ms": round(float(np.median(ms)), 3),
                          "uniform_general_launches": launches}), flush=True)


if __name__ == "__main__":
    main()
