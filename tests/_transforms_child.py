"""Child process of tests/test_gpu_transforms.py: the 20000-particle frame
comparison (a handle with a frame against a frame-less handle fed the
rewritten arrays; eager, one-call host and one-call device selections, with
and without a Sphere) under whatever PBX_* runtime variables the parent set
— they are read once per process.  Exits non-zero on the first difference."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "pynbody-extras_amd"), str(ROOT / "tests")]

from pynbodyext import _native as nat  # noqa: E402


def main() -> None:
    import test_gpu_transforms as t

    nat.load()
    nat.set_device(0)
    for kind in ("eager", "lazy", "ondev"):
        for sphere in (t.SPHERE, None):
            p = t.Pair(20000, "all", kind, sphere=sphere)
            try:
                t.compare_pair(p)
            finally:
                p.close()
    print("frame pairs identical")


if __name__ == "__main__":
    main()
