"""The numpy restatement of the final reduction's two summation orders (tests/reduce_numpy.py) against exact arithmetic: Python integers on integer-valued
partials, math.fsum on random doubles.  tests/test_gpu_reduce_final.py then holds the device to the restatement bit for bit.

Depth, counted from the restatement's own tree (reduce_numpy.depth: the longest chain of rounded additions a partial passes through; additions of a structural zero --
an accumulator's initial 0.0, a missing partial, an accumulator or lane that received nothing -- are exact and not counted):
  small: (partials of the fullest lane - 1) + the exchanges and row additions that meet a second number, at most 4 + 2.
         1 block: 0, 2: 1, 63 and 64: 6, 65 and 127: 7, 1023 and 1024: 15 + 6 = 21.
  large: (partials of the fullest accumulator - 1) + at most 2 to combine the accumulators + 6 shuffles + 15 wave additions.  Left-over partials of a class all go to s0, so
         the depth is not monotone in the count: 1025..2048 blocks: 22, 2049..4096: 23, 4097: 24, 5121: 25, 7168 and 7169: 26 (s0 holds 1 + 3), 8191 and 8192: 24, 8193: 25,
         12289: 26, 15360 and 15361: 28 (s0 holds 3 + 3), 16384: 26, 16385: 27, 20481: 28.
The accuracy bound is (depth + 1) * 2^-53 * sum |p|: depth * u to first order, the + 1 covers the higher orders (depth * u < 2^-48)."""
import math

import numpy as np
import pytest

import reduce_numpy as rn

# depth of final() at every count of the list, as the docstring states them
DEPTHS = {1: 0, 2: 1, 63: 6, 64: 6, 65: 7, 127: 7, 1023: 21, 1024: 21, 1025: 22, 2047: 22, 2048: 22, 2049: 23, 3072: 23, 3073: 23, 4095: 23, 4096: 23, 4097: 24, 5121: 25,
          7168: 26, 7169: 26, 8191: 24, 8192: 24, 8193: 25, 12289: 26, 15360: 28, 15361: 28, 16384: 26, 16385: 27, 20481: 28}
NVALS = (1, 2, 3, 5, 8)


def forms(n):
    return (("small", rn.small), ("large", rn.large), ("final", rn.final)) if n <= rn.FB else (("large", rn.large), ("final", rn.final))


def test_the_list_of_counts_and_the_stated_depths():
    assert set(DEPTHS) == set(rn.NBLOCKS) and len(rn.NBLOCKS) == 29
    for n in rn.NBLOCKS:
        assert rn.depth(n) == DEPTHS[n], (n, rn.depth(n))
        assert rn.depth(n, "large") <= 28
    assert rn.depth(1024, "small") == 21 and rn.depth(1024, "large") == 21 and rn.depth(1025, "large") == 22


@pytest.mark.parametrize("n", rn.NBLOCKS)
def test_integer_partials_sum_exactly_in_both_forms_and_layouts(n):
    rng = np.random.default_rng(1000 + n)
    for nvals in NVALS:
        ints = rng.integers(-(2 ** 20) + 1, 2 ** 20, size=(n, nvals))
        p = ints.astype(np.float64)
        for v in range(nvals):
            want = sum(int(x) for x in ints[:, v])
            for name, f in forms(n):
                for soa in (False, True):
                    assert f(p, v, soa) == want, (name, n, nvals, v, soa)


@pytest.mark.parametrize("n", rn.NBLOCKS)
def test_random_doubles_within_the_depth_bound_of_fsum_and_layouts_agree(n):
    rng = np.random.default_rng(2000 + n)
    for nvals in NVALS:
        p = rng.standard_normal((n, nvals)) * np.exp2(rng.uniform(-20, 20, size=(n, nvals)))
        for v in range(nvals):
            exact, total = math.fsum(p[:, v]), math.fsum(np.abs(p[:, v]))
            for name, f in forms(n):
                got = f(p, v, False)
                d = rn.depth(n, name)
                assert abs(got - exact) <= (d + 1) * 2.0 ** -53 * total, (name, n, nvals, v, got - exact, d)
                assert f(p, v, True) == got, (name, n, nvals, v)


def test_a_single_changed_partial_changes_the_sum():
    """every position is read exactly once: bumping one integer partial by one moves the sum by one (a dropped, doubled or mis-strided read would not)"""
    for n in (65, 1024, 1025, 4097, 20481):
        for nvals, v in ((1, 0), (3, 1), (5, 4)):
            p = np.zeros((n, nvals))
            base = rn.final(p, v)
            for i in {0, 1, 63, 64, n // 2, n - 2, n - 1}:
                q = p.copy()
                q[i, v] = 1.0
                q[i, (v + 1) % nvals] += 2.0 if nvals > 1 else 0.0
                for soa in (False, True):
                    assert rn.final(q, v, soa) == base + 1.0, (n, nvals, v, i, soa)


def test_non_finite_partials_propagate():
    for n in (127, 5121):
        p = np.ones((n, 2))
        p[-1, 1] = np.nan
        assert rn.final(p, 0) == n and math.isnan(rn.final(p, 1)) and math.isnan(rn.final(p, 1, True))
        p[-1, 1] = np.inf
        assert rn.final(p, 1) == np.inf and rn.final(p, 1, True) == np.inf
