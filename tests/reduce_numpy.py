"""Numpy restatement of the two summation orders of the one-block final reduction (csrc/blas.hip reduce_final behind reduce_to_slot; the orders themselves:
csrc/lqcd_internal.h sum_partials_small_nv + wave_sum for at most 1024 block partials, sum_partials_class + shfl_tree_sum + the sixteen wave sums for more),
written from the comments and the code in plain float64 additions.  This stage has a fixed order and no fmas, so numpy gives the bits of the device:
"the same bits" in those comments means equality with final() below.

A reduction holds `nvals` values per block.  partials is the logical array [nblocks][nvals]; flatten() gives its memory image, interleaved ([block][value]) or
soa ([value][block]), and every function reads the image through the kernel's own index expression -- a wrong stride reads a wrong number here as it does there.

small   lane l of one wave adds the partials l, l + 64, ..., l + 64 * 15 to 0.0 in sequence (a missing one is +0.0), then wave_sum: four exchanges inside the
        16-lane rows (lane ^ 1, lane ^ 2, mirror of the 8-lane half row, mirror of the row), then (r0 + r16) + (r32 + r48).
large   thread c of 1024 owns the partials c, c + 1024, ...: while c' + 3 * 1024 < nblocks four of them go to the accumulators s0, s1, s2, s3, the up to three left
        over go to s0, the class sum is (s0 + s1) + (s2 + s3) (the plain loops of sum_partials_class; its 8- and 16-load loops promise the same additions);
        the 64 class sums of a wave go through the __shfl_down tree (offsets 32, 16, ..., 1), the sixteen wave sums are added to 0.0 in sequence.
final   small for nblocks <= 1024, large above.

depth() runs the same tree on addition counts instead of numbers: the longest chain of ROUNDED additions a partial passes through (adding to an accumulator that
still holds its initial zero, and adding a missing partial's +0.0, is exact and not counted).  The error of a sum is at most depth * 2^-53 * sum |p| to first order."""
import numpy as np

FB = 1024          # threads of the one block; more partials than this take the large form
# every boundary of the lane loop (64), of the small / large switch (1024) and of the 4-, 8- and 16-load loops (3072, 7168, 15360), each with a ragged neighbour
NBLOCKS = (1, 2, 63, 64, 65, 127, 1023, 1024, 1025, 2047, 2048, 2049,
           3072, 3073, 4095, 4096, 4097, 5121,
           7168, 7169, 8191, 8192, 8193, 12289,
           15360, 15361, 16384, 16385, 20481)


def flatten(partials, soa):
    """memory image of partials[nblocks][nvals]: [block][value], or [value][block] with soa"""
    p = np.asarray(partials, dtype=np.float64)
    assert p.ndim == 2
    return np.ascontiguousarray(p.T if soa else p).reshape(-1)


class _Values:
    """float64 arithmetic, one rounding per addition"""
    @staticmethod
    def zeros(n):
        return np.zeros(n, dtype=np.float64)

    @staticmethod
    def load(flat, idx, present):
        return np.where(present, flat[np.where(present, idx, 0)], 0.0)

    @staticmethod
    def add(a, b):
        with np.errstate(invalid="ignore", over="ignore"):
            return np.add(a, b, dtype=np.float64)


class _Depths:
    """the same tree on counts: EMPTY marks a structural zero (adding it is exact), a partial starts at 0, a rounded addition gives max + 1"""
    EMPTY = -1

    @staticmethod
    def zeros(n):
        return np.full(n, _Depths.EMPTY, dtype=np.int64)

    @staticmethod
    def load(flat, idx, present):
        return np.where(present, 0, _Depths.EMPTY).astype(np.int64)

    @staticmethod
    def add(a, b):
        a, b = np.asarray(a), np.asarray(b)
        return np.where(a < 0, b, np.where(b < 0, a, np.maximum(a, b) + 1))


def _index(i, v, n, nvals, soa):
    return v * n + i if soa else i * nvals + v


def _small(flat, n, nvals, v, soa, A):
    assert 1 <= n <= 16 * 64
    lane = np.arange(64)
    s = A.zeros(64)
    for k in range(16):
        i = lane + 64 * k
        s = A.add(s, A.load(flat, _index(i, v, n, nvals, soa), i < n))
    for src in (lane ^ 1, lane ^ 2, (lane & ~7) | (7 - (lane & 7)), (lane & ~15) | (15 - (lane & 15))):
        s = A.add(s, s[src])
    return A.add(A.add(s[0], s[16]), A.add(s[32], s[48]))


def _large(flat, n, nvals, v, soa, A):
    assert n >= 1
    c = np.arange(FB)
    s = [A.zeros(FB) for _ in range(4)]

    def step(q, i):      # s[q] += partial i, for the classes that have one there
        m = i < n
        s[q] = np.where(m, A.add(s[q], A.load(flat, _index(i, v, n, nvals, soa), m)), s[q])

    i = c.copy()
    while (i + 3 * FB < n).any():
        four = i + 3 * FB < n                                   # these classes take four partials in this round ...
        for q in range(4):
            step(q, np.where(four, i + q * FB, n))
        i = np.where(four, i + 4 * FB, i)
    for _ in range(3):                                          # ... the others are in the tail: one partial at a time into s0
        step(0, i)
        i = i + FB
    assert (i >= n).all()
    cls = A.add(A.add(s[0], s[1]), A.add(s[2], s[3]))
    w = cls.reshape(FB // 64, 64).copy()
    off = 32
    while off:
        w[:, :off] = A.add(w[:, :off], w[:, off:2 * off])
        off >>= 1
    t = A.zeros(1)[0]
    for k in range(FB // 64):
        t = A.add(t, w[k, 0])
    return t


def _run(tree, partials, v, soa):
    p = np.asarray(partials, dtype=np.float64)
    n, nvals = p.shape
    assert 0 <= v < nvals
    return float(tree(flatten(p, soa), n, nvals, v, soa, _Values))


def small(partials, v=0, soa=False):
    return _run(_small, partials, v, soa)


def large(partials, v=0, soa=False):
    return _run(_large, partials, v, soa)


def final(partials, v=0, soa=False):
    return small(partials, v, soa) if len(partials) <= FB else large(partials, v, soa)


def depth(nblocks, form="final"):
    tree = {"small": _small, "large": _large, "final": _small if nblocks <= FB else _large}[form]
    return int(tree(None, nblocks, 1, 0, False, _Depths))
