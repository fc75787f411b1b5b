"""The residual ring at depths 16 and 32 (cg_rring x cg_rring_mult; cg.hip cg_batch_px<NT, DEPTH>, cg_run's captured burst) restated in numpy: no GPU.

Extends the model of tests/test_cpu_cg_recurrence.py (imported, not edited): histories of 32 entries indexed by (S_ITERS - S_BSTART) & 31, a done flag
behind which every launch is a no-op, and an iteration that takes its slot role m as an argument -- what a replayed burst does: the roles of the captured
iterations are baked in.  Pinned here, before any kernel runs: the history index and S_BSTART of every iteration, the slot each iteration reads and
writes, the flush at every np = 1 .. depth, windows of every length up to 2 depth + 2 against the oracle's fixed-window CG (1e-12, the bound the forms
hold among themselves), a burst rounded up to the depth against plain enqueueing (same iterate, same count; a burst of 8 at depth 16 is NOT), and the
stopping rows of tests/test_gpu_cg_rring_deep.py: the oracle stops at it == k at the eps chosen for them and the last update is visible."""
import numpy as np
import pytest

import rring_deep as rd
import solve_endings as se
from test_cpu_cg_recurrence import BC, KAPPA, RingCG

RMAX = 32


class DeepRingCG(RingCG):
    def __init__(self, orc, U, b, L, depth, eps=-1.0):
        super().__init__(orc, U, b, L, depth)
        self.ah = [0.0] * RMAX
        self.bh = [0.0] * RMAX
        self.eps = eps
        self.done = False
        self.log = []          # (k, m, history index, S_BSTART, slot read, slot written, pending terms applied by the batch launch)

    def iterate(self, m=None):
        """one enqueued iteration with the slot role m (None: k % depth, what cg_enqueue_rring computes; a replay passes the captured one)"""
        K = self.K
        m = self.k % K if m is None else m
        self.k += 1
        if self.done:                                             # every launch behind the converging iteration is a no-op
            return
        applied = 0
        if m == 0:
            applied = self.iters - self.bstart
            if applied > 0:
                assert applied == K, (applied, K)                 # cg_batch_px, fin = 0: a full batch or nothing
                self.x, self.p = self.batch(self.x, self.p, False)
            self.s = self.D(self.p)
            self.bstart = self.iters                              # op 9
        else:
            self.s = self.D(self.slots[m]) + self.beta * self.s
        j = (self.iters - self.bstart) & (RMAX - 1)
        al = self.rr / float(np.vdot(self.s, self.s).real)
        self.ah[j] = al
        rn = self.slots[m] - al * self.D(self.s, True)
        self.slots[(m + 1) % K] = rn
        rrn = float(np.vdot(rn, rn).real)
        self.beta = rrn / self.rr
        self.bh[j] = self.beta
        self.rr = rrn
        self.log.append((self.iters, m, j, self.bstart, m, (m + 1) % K, applied))
        self.iters += 1
        if rrn < self.eps:
            self.done = True


def system(orc, L):
    return orc.hot_gauge(L, 111), orc.gaussian_spinor(orc.wilson_shape(L), 112)


@pytest.mark.parametrize("depth", rd.DEPTHS)
def test_windows_of_every_length_and_the_bookkeeping(orc, depth):
    L = (4, 4, 4, 4)
    U, b = system(orc, L)
    cg = DeepRingCG(orc, U, b, L, depth)
    worst = 0.0
    for n in range(1, 2 * depth + 3):
        cg.iterate()
        k, m, j, bstart, src, dst, applied = cg.log[-1]
        assert k == n - 1 and m == k % depth and j == k % depth < depth and bstart == k - k % depth
        assert (src, dst) == (k % depth, (k + 1) % depth)
        assert applied == (depth if m == 0 and k > 0 else 0)
        assert cg.iters - cg.bstart == (n - 1) % depth + 1                     # np of a flush here: every value 1 .. depth comes by
        got = cg.flushed_x()
        ref = orc.cg_DdagD_fixed(orc.WILSON, U, b, L, KAPPA, 1.0, BC, niter=n)
        err = rd.relmax(got, ref)
        worst = max(worst, err)
        assert err <= 1e-12, (depth, n, err)
    assert {e[2] for e in cg.log} == set(range(depth))
    print("depth", depth, "largest rel max diff over windows 1..%d: %.3e" % (2 * depth + 2, worst))


def burst_length(depth, check_every=8):
    """cg_run: the captured burst is the multiple of the depth at or above check_every"""
    return (check_every + depth - 1) // depth * depth


def run(cg, maxiter, blen, replay):
    """cg_run's loop: bursts of blen while that many iterations are left (replay: the roles of the first burst, as a captured graph has them), the
    rest enqueued plainly; the scalars are read back between bursts"""
    roles = None
    it = 0
    while not cg.done and it < maxiter:
        burst = min(blen, maxiter - it)
        if replay and burst == blen:
            if roles is None:
                roles = [(cg.k + i) % cg.K for i in range(burst)]
            for m in roles:
                cg.iterate(m)
        else:
            for _ in range(burst):
                cg.iterate()
        it = cg.iters
    return cg.flushed_x(), cg.iters


@pytest.mark.parametrize("depth", [2, 4, 8, 16, 32])
def test_a_burst_rounded_up_to_the_depth_replays_like_plain_enqueueing(orc, depth):
    assert burst_length(depth) == (8 if depth <= 8 else depth) and burst_length(depth) % depth == 0
    L = (4, 4, 4, 4)
    U, b = system(orc, L)
    rr0 = float(np.vdot(b, b).real)
    for eps, maxiter in ((-1.0, 3 * depth + 5), (-1.0, 2 * burst_length(depth)), (1e-9 * rr0, 400), (1e-4 * rr0, 400)):
        plain = run(DeepRingCG(orc, U, b, L, depth, eps), maxiter, 8, False)
        graph = run(DeepRingCG(orc, U, b, L, depth, eps), maxiter, burst_length(depth), True)
        assert plain[1] == graph[1] and np.array_equal(plain[0], graph[0]), (depth, eps, maxiter)
        assert plain[1] == maxiter if eps < 0 else 0 < plain[1] < maxiter
    if depth > 8:      # the model can tell: a burst of 8 replayed at this depth finds the ring elsewhere
        plain = run(DeepRingCG(orc, U, b, L, depth), 3 * depth, 8, False)
        with pytest.raises(AssertionError):
            bad = run(DeepRingCG(orc, U, b, L, depth), 3 * depth, 8, True)
            assert np.array_equal(plain[0], bad[0])


# the last update of a stopping row must be visible above the 1e-10 the device is held to: a flush one term short then misses the bound by this factor
VISIBLE = 100 * 1e-10


@pytest.mark.parametrize("r", rd.ending_rows(), ids=lambda r: r["name"])
def test_the_oracle_stops_the_ending_rows_at_k(orc, r):
    sc, x, it, st = rd.ending(orc, r)
    hi, lo = se.separated(r, sc)
    print("%s eps %.6e: %.3f below rr_{k-1}, %.3f above rr_k" % (r["name"], sc["eps"], hi / sc["eps"], sc["eps"] / lo))
    assert hi / sc["eps"] >= se.MARGIN and sc["eps"] / lo >= se.MARGIN
    assert st == 0 and it == r["k"], (it, r["k"])
    assert np.array_equal(x, se.capped(orc, r, r["k"])[0])
    last = se.rel_err(x, se.capped(orc, r, r["k"] - 1)[0])
    trunc = se.rel_err(x, se.solve(orc, r, se.TIGHT)[0])
    print("  last update %.3e, truncation error %.3e" % (last, trunc))
    assert last >= VISIBLE and trunc >= VISIBLE
