"""The one-block final reduction behind every solver scalar (csrc/blas.hip reduce_final through reduce_to_slot), called directly on host partials through
lqcd_bench_reduce_partials and held to tests/reduce_numpy.py bit for bit: that restatement is what "the same bits" in the comments of csrc/lqcd_internal.h means.
Counts: every boundary of the lane loop, of the small / large switch and of the 4-, 8- and 16-load loops of sum_partials_class, each with a ragged neighbour
(reduce_numpy.NBLOCKS), crossed with 1, 2, 3, 5 and 8 values per block and both layouts of the partials.  The hook keeps 64 NaNs behind the partials on the
device, so a loop bound that reads one partial too many shows as a NaN sum.

Out of scope here: the sum over ranks inside the block (pr.nranks > 0, the peer-mapped backend) and the CG / BiCGStab scalar steps behind the sum (cg_op): the hook
calls reduce_to_slot without an all-reduce and with cg_op = 0."""
import ctypes as C
import math

import numpy as np
import pytest

import reduce_numpy as rn

pytestmark = pytest.mark.gpu

NVALS = (1, 2, 3, 5, 8)
SENTINEL = -1.2345e300      # LQCD_BENCH_REDUCE_SENTINEL (include/lqcd_hip.h)


@pytest.fixture(scope="module")
def lat(lq):
    assert lq.lib.device_count() > 0, "no HIP device visible: the product has no CPU fallback"
    return lq.Lattice((4, 4, 4, 4))


def status(lq, lat, flat, nblocks, nvals, soa, out, guard):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    return lq.lib.lib().lqcd_bench_reduce_partials(lat._h, ptr(flat), int(nblocks), int(nvals), int(soa), ptr(out), ptr(guard))


def reduce(lq, lat, partials, soa):
    """the device's sums of partials[nblocks][nvals], laid out as the kernel will read them; the guard slots are checked on every call"""
    n, nvals = partials.shape
    out, guard = np.full(nvals, 4711.0), np.zeros(2)
    lq.lib.check(status(lq, lat, rn.flatten(partials, soa), n, nvals, soa, out, guard))
    assert guard[0] == SENTINEL and guard[1] == SENTINEL, (n, nvals, soa, guard)
    return out


def integer_partials(n, nvals):
    """a different stream per value (|p| < 2^20, so every sum is exact in any order): a value read with another value's stride or offset gives another sum"""
    rng = np.random.default_rng(31 * n + nvals)
    return rng.integers(-(2 ** 20) + 1, 2 ** 20, size=(n, nvals))


def random_partials(n, nvals):
    rng = np.random.default_rng(77 * n + nvals)
    return rng.standard_normal((n, nvals)) * np.exp2(rng.uniform(-20, 20, size=(n, nvals)))


@pytest.mark.parametrize("soa", [0, 1])
@pytest.mark.parametrize("nvals", NVALS)
@pytest.mark.parametrize("n", rn.NBLOCKS)
def test_sums_are_exact_on_integers_and_the_bits_of_the_restatement_on_doubles(lq, lat, n, nvals, soa):
    ints = integer_partials(n, nvals)
    got = reduce(lq, lat, ints.astype(np.float64), soa)
    for v in range(nvals):
        assert got[v] == sum(int(x) for x in ints[:, v]), (n, nvals, soa, v)
    p = random_partials(n, nvals)
    got = reduce(lq, lat, p, soa)
    again = reduce(lq, lat, p, soa)
    for v in range(nvals):
        want = rn.final(p, v, bool(soa))
        assert got[v] == want, (n, nvals, soa, v, got[v] - want)
        assert again[v] == got[v] and math.copysign(1.0, again[v]) == math.copysign(1.0, got[v])


@pytest.mark.parametrize("soa", [0, 1])
@pytest.mark.parametrize("n", [127, 5121])
def test_a_non_finite_last_partial_gives_a_non_finite_sum_of_its_kind(lq, lat, n, soa):
    for nvals in (1, 3, 8):
        p = integer_partials(n, nvals).astype(np.float64)
        v = nvals - 1
        exact = [float(p[:, k].sum()) for k in range(nvals)]
        p[n - 1, v] = np.nan
        got = reduce(lq, lat, p, soa)
        assert math.isnan(got[v]) and list(got[:v]) == exact[:v], (n, nvals, got)
        p[n - 1, v] = np.inf
        got = reduce(lq, lat, p, soa)
        assert got[v] == np.inf and list(got[:v]) == exact[:v], (n, nvals, got)


def test_refusals_leave_the_output_untouched(lq, lat):
    flat, guard = np.ones(16), np.zeros(2)
    for nblocks, nvals, f, o, g in ((2, 0, flat, True, guard), (2, 9, flat, True, guard), (0, 2, flat, True, guard), (-3, 1, flat, True, guard),
                                    (2, 2, None, True, guard), (2, 2, flat, True, None), (2, 2, flat, False, guard)):
        out = np.full(8, 4711.0)
        st = status(lq, lat, f, nblocks, nvals, 0, out if o else None, g)
        assert st == lq.lib.ERR_ARG, (nblocks, nvals, st)
        assert (out == 4711.0).all() and (guard == 0.0).all()
    out = np.full(8, 4711.0)
    assert lq.lib.lib().lqcd_bench_reduce_partials(None, flat.ctypes.data_as(C.POINTER(C.c_double)), 2, 2, 0, out.ctypes.data_as(C.POINTER(C.c_double)),
                                                   guard.ctypes.data_as(C.POINTER(C.c_double))) == lq.lib.ERR_ARG
    assert (out == 4711.0).all()
    # ... and the context still reduces: a dot product through the same slots
    assert list(reduce(lq, lat, np.arange(12.0).reshape(6, 2), 0)) == [30.0, 36.0]
