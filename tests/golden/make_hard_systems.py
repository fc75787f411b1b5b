"""Generates tests/golden/hard_systems.json: what the oracle's textbook solvers show on every row of tests/hard_systems.SYSTEMS -- iteration count,
recursive residual, true residual, |x|, |b| and the constant C_ref of the accuracy contract (tests/hard_systems.py).  Scalars only.  The GPU tests
read the file instead of rerunning the oracle's long solves; tests/test_cpu_hard_system_reference.py checks that it is current.

    python tests/golden/make_hard_systems.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import hard_systems as hs  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def main():
    orc.build()
    out = {}
    for name, s in hs.SYSTEMS.items():
        out[name] = hs.reference(orc, s)
        print(name, out[name])
    with open(hs.FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
