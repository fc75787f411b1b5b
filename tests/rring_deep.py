"""The deep residual ring (cg_fused = 3 with cg_rring_mult = M > 1: K M = 16 or 32 slots; cg.hip cg_batch_px<NT, DEPTH>): the cases shared by
tests/test_cpu_cg_recurrence_deep.py (the oracle side, no GPU) and tests/test_gpu_cg_rring_deep.py (the device side).

Systems.  Fixed windows run on smooth links at kappa = 0.1285 with periodic boundaries (tests/hard_systems.py: a solve takes ~1000 iterations, so the
updates of iteration 3 d + 5 still matter; on the hot-start system of the other ring tests the solve has converged by then).  Endings run on the hot
system of tests/solve_endings.py, where the oracle can place an eps between two residuals five decades above the bound.
"""
import numpy as np

import hard_systems as hs
import solve_endings as se

SMALL, BIG = (16, 8, 8, 4), (16, 16, 16, 8)
LATTICES = (SMALL, BIG)
KM = ((8, 2), (4, 4), (8, 4))      # (cg_rring, cg_rring_mult): depths 16, 16, 32
DEPTHS = (16, 32)


def windows(d):
    """below, at and above one and two batch boundaries, and inside the fourth batch"""
    return (1, d - 1, d, d + 1, 2 * d - 1, 2 * d, 2 * d + 1, 3 * d + 5)


ALL_WINDOWS = tuple(sorted({n for d in DEPTHS for n in windows(d)}))


def smooth(L):
    """the kappa = 0.1285 row of tests/hard_systems.py at the shape L (the 16.8.8.4 one is its wilson_cg_16)"""
    L = tuple(L)
    if L == SMALL:
        return hs.system("wilson_cg_16")
    return dict(kind="wilson", solver="cg", L=L, kappa=0.1285, bc=hs.PERIODIC, source="gauss", seed=7, eps=hs.EPS, name="wilson_cg_" + ".".join(str(v) for v in L))


def ending_ks(d):
    """stopping iterations with k mod d = d - 1, 0, 1: the flush of a full batch but one term, of a full batch behind a batch launch that was a no-op, of one term"""
    return (d - 1, d, d + 1)


def ending_rows():
    return [se._row("wilson", "cg", L, k)[1] for L in LATTICES for d in DEPTHS for k in ending_ks(d)]


_memo = {}


def ending(orc, r):
    """(eps, x, iterations) of the oracle for the row: eps in the (geometric) middle of rr_{k-1} and rr_k, its solve at that eps.  Memoised, read-only."""
    if r["name"] not in _memo:
        sc = se.select(orc, r)
        x, it, rr, st = se.solve(orc, r, sc["eps"])
        x.setflags(write=False)
        _memo[r["name"]] = (sc, x, int(it), int(st))
    return _memo[r["name"]]


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())
