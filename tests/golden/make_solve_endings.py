"""Generates tests/golden/solve_endings.json: for every row of tests/solve_endings.ROWS the oracle's residuals around the target iteration and the eps
placed between them (k, eps, rr_km1, rr_k, ss_k).  Scalars only; tests/test_cpu_solve_endings.py checks that the file is current and that every row
meets the conditions it is there for.  Prints, per row, the margins of eps to the two residuals it separates.

    python tests/golden/make_solve_endings.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import solve_endings as se  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def main():
    orc.build()
    out = {}
    for name, r in se.ROWS.items():
        sc = se.select(orc, r)
        out[name] = sc
        if sc["eps"] is None:
            print("%-48s NO HALF STEP  rr_km1 %.4e rr_k %.4e" % (name, sc["rr_km1"], sc["rr_k"]))
            continue
        hi, lo = se.separated(r, sc)
        print("%-48s eps %.4e  above %.3g  below %.3g%s" % (name, sc["eps"], hi / sc["eps"], sc["eps"] / lo, "" if min(hi / sc["eps"], sc["eps"] / lo) >= se.MARGIN else "   <-- MARGIN"))
    with open(se.FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
