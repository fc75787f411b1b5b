"""The residual-ring form of the fp64 CG on D^+D (cg_fused = 3, cg.hip cg_batch_px / cg_enqueue_rring) restated in numpy on the oracle's Wilson operator: no GPU.

s_k = D p_k is formed by the recurrence s_{k+1} = D r_{k+1} + beta_k s_k and restarted from an exact D p at every batch boundary; the K residuals of a batch stay
in a ring of K slots (r_k in slot k % K); alpha_k and beta_k go to histories; p and x are brought up to date once per K iterations by x += alpha_j p, p = r_{j+1} +
beta_j p over the pending iterations, oldest first; a window that ends inside a batch applies the pending alpha p terms to x and forms no last p.  This pins the
bookkeeping (histories, slots, partial batches) before any kernel runs: windows of every length 1..20 equal the oracle's fixed-window CG to 1e-12 (the bound the
GPU forms hold among themselves; the restatement differs from the textbook recurrence by the rounding of s alone)."""
import numpy as np
import pytest

KAPPA = 0.141139
BC = (1, 1, 1, -1)


class RingCG:
    def __init__(self, orc, U, b, L, K):
        self.D = lambda v, dag=False: orc.wilson_D(U, v, L, KAPPA, 1.0, BC, dagger=dag)
        self.K = K
        self.x = np.zeros_like(b)
        self.slots = [None] * K
        self.slots[0] = b.copy()            # x0 = 0: r_0 = b
        self.p = b.copy()
        self.s = None
        self.rr = float(np.vdot(b, b).real)
        self.iters = 0                      # S_ITERS
        self.bstart = 0                     # S_BSTART
        self.ah = [0.0] * 8
        self.bh = [0.0] * 8
        self.beta = 0.0
        self.k = 0

    def batch(self, x, p, final):
        """cg_batch_px: returns the new (x, p); p is None for a final flush"""
        n = self.iters - self.bstart
        x, p = x.copy(), p.copy()
        for j in range(n):
            x = x + self.ah[j] * p
            if not final or j < n - 1:
                p = self.slots[(j + 1) % self.K] + self.bh[j] * p
        return x, (None if final else p)

    def iterate(self):
        K, m = self.K, self.k % self.K
        if m == 0:
            if self.iters - self.bstart > 0:
                assert self.iters - self.bstart == K
                self.x, self.p = self.batch(self.x, self.p, False)
            self.s = self.D(self.p)                               # plain D on the fresh p: the recurrence restarts
            self.bstart = self.iters
        else:
            self.s = self.D(self.slots[m]) + self.beta * self.s   # recurrence mode
        j = self.iters - self.bstart
        al = self.rr / float(np.vdot(self.s, self.s).real)
        self.ah[j] = al
        rn = self.slots[m] - al * self.D(self.s, True)            # update-mode D^+: slot m -> slot m + 1
        self.slots[(m + 1) % K] = rn
        rrn = float(np.vdot(rn, rn).real)
        self.beta = rrn / self.rr
        self.bh[j] = self.beta
        self.rr = rrn
        self.iters += 1
        self.k += 1

    def flushed_x(self):
        """what cg_flush_x leaves in x (the state of the window is not touched)"""
        return self.batch(self.x, self.p, True)[0]


@pytest.mark.parametrize("L", [(4, 4, 4, 4), (8, 4, 4, 4)])
@pytest.mark.parametrize("K", [2, 4, 8])
def test_windows_of_every_length_equal_the_fixed_window_cg(orc, L, K):
    U = orc.hot_gauge(L, 111)
    b = orc.gaussian_spinor(orc.wilson_shape(L), 112)
    cg = RingCG(orc, U, b, L, K)
    worst = 0.0
    for n in range(1, 21):
        cg.iterate()
        got = cg.flushed_x()
        ref = orc.cg_DdagD_fixed(orc.WILSON, U, b, L, KAPPA, 1.0, BC, niter=n)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        worst = max(worst, err)
        assert err <= 1e-12, (L, K, n, err)
    print("L", L, "K", K, "largest rel max diff over windows 1..20: %.3e" % worst)
