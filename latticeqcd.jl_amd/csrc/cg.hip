// cg.hip -- CG on D^+D with device-resident scalars: the iteration forms (reference, |D p|^2 fused, fully fused with the x update every iteration or deferred,
// small-lattice, residual ring), temporal gauge, the generic CG on an enqueue function and the staggered parity-block solve.
//
// Replaces, behind the C ABI, LatticeDiracOperators.jl's solve_DinvX!(y, DdagD, x) (cg) -- SURVEY.md 8(a) a4.
#include "ops_internal.h"
#include "stencil_common.h"      // HArgs, wilson_pack_axpy_block: pack blocks appended to the x/p update launch (partitioned lattices)

#include <algorithm>
#include <cmath>

namespace lqcd {

// ---------------------------------------------------------------------------------- CG with device-resident scalars

__global__ void cg_scalar_alpha(double* s) {
    if (s[S_DONE] != 0.0) { s[S_XDONE] = 1.0; return; }   // the iterate of the converging iteration has been written
    s[S_ALPHA] = s[S_RR] / s[S_PQ];
}
__global__ void cg_scalar_beta(double* s) {
    if (s[S_DONE] != 0.0) return;
    const double rrn = s[S_RRNEW];
    s[S_BETA] = rrn / s[S_RR];
    s[S_RR] = rrn;
    s[S_ITERS] += 1.0;
    if (rrn < s[S_EPS]) s[S_DONE] = 1.0;
}

// x += alpha p ; r -= alpha q ; partial |r|^2
__global__ __launch_bounds__(UB) void cg_update_xr(const double* __restrict__ s, double2* __restrict__ x, double2* __restrict__ r,
                                                    const double2* __restrict__ p, const double2* __restrict__ q, size_t n,
                                                    double* partial) {
    __shared__ double red[UB / 64];
    double acc = 0;
    if (s[S_DONE] == 0.0) {
        const double al = s[S_ALPHA];
        for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
            const double2 pv = p[i], qv = q[i];
            double2 xv = x[i], rv = r[i];
            xv.x = fma(al, pv.x, xv.x); xv.y = fma(al, pv.y, xv.y);
            rv.x = fma(-al, qv.x, rv.x); rv.y = fma(-al, qv.y, rv.y);
            x[i] = xv; r[i] = rv;
            acc = fma(rv.x, rv.x, acc); acc = fma(rv.y, rv.y, acc);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0;
        for (int w = 0; w < UB / 64; w++) t += red[w];
        partial[blockIdx.x] = t;
    }
}
// fused tail of an iteration:  x += alpha p ;  p = r + beta p   (x is still updated in the iteration that converges,
// p only while the solve continues; nothing is touched in later, overshooting launches)
__global__ __launch_bounds__(UB) void cg_update_xp(const double* __restrict__ s, double2* __restrict__ x, double2* __restrict__ p,
                                                    const double2* __restrict__ r, size_t n) {
    if (s[S_XDONE] != 0.0) return;
    const double al = s[S_ALPHA], be = s[S_BETA];
    const bool cont = s[S_DONE] == 0.0;
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        double2 pv = p[i], xv = x[i];
        xv.x = fma(al, pv.x, xv.x); xv.y = fma(al, pv.y, xv.y);
        x[i] = xv;
        if (cont) {
            const double2 rv = r[i];
            pv.x = fma(be, pv.x, rv.x); pv.y = fma(be, pv.y, rv.y);
            p[i] = pv;
        }
    }
}
// cg_small: the same tail with the second reduction folded in.  Every wave sums the block partials of |r|^2 the update-mode stencil left
// (reduce_final's order), forms beta = rr' / rr (rr = the value this iteration started from, S_RROLD: nobody writes it here) and the
// convergence test itself; block 0 records rr', beta, the iteration count and the done flag for the kernels behind this one.
__global__ __launch_bounds__(UB) void cg_update_xp_small(double* __restrict__ s, double2* __restrict__ x, double2* __restrict__ p,
                                                          const double2* __restrict__ r, size_t n, const double* __restrict__ part, int nb) {
    if (s[S_XDONE] != 0.0) return;
    const double rrn = sum_partials_small(part, nb);
    const double al = s[S_ALPHA], be = rrn / s[S_RROLD];
    const bool cont = !(rrn < s[S_EPS]);
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        double2 pv = p[i], xv = x[i];
        xv.x = fma(al, pv.x, xv.x); xv.y = fma(al, pv.y, xv.y);
        x[i] = xv;
        if (cont) {
            const double2 rv = r[i];
            pv.x = fma(be, pv.x, rv.x); pv.y = fma(be, pv.y, rv.y);
            p[i] = pv;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        s[S_RRNEW] = rrn;
        s[S_BETA] = be;
        s[S_RR] = rrn;
        s[S_ITERS] += 1.0;
        if (!cont) s[S_DONE] = 1.0;
    }
}
// Deferred x update (cg_defer_x): iteration k even:  p_{k+1} = r + beta p_k into the OTHER buffer, x untouched, alpha_k kept;
//                                    iteration k odd:   x += alpha_{k-1} p_{k-1} + alpha_k p_k (same order of operations as two single
// updates: identical bits), p_{k+1} = r + beta p_k over the dead p_{k-1}.  3 + 6 streams per pair of iterations instead of 5 + 5.  The
// iteration that converges completes x itself; nothing is touched in later, overshooting launches.
// FOLD (several ranks): the scalar step behind the second all-reduce (beta = rr'/rr, rr = rr', iteration count, convergence flag) is done here --
// every block forms beta and the test from the all-reduced rr' (S_RRNEW) and the rr this iteration started from (S_RROLD, written by the
// update-mode stencil), block 0 records the results -- instead of by a one-thread kernel between the all-reduce and this launch.
struct FoldBeta { double be; bool cont; };
template <bool FOLD>
__device__ inline FoldBeta cg_beta(double* s) {
    FoldBeta f;
    if constexpr (FOLD) {
        const double rrn = s[S_RRNEW];
        f.be = rrn / s[S_RROLD];
        f.cont = !(rrn < s[S_EPS]);
    } else {
        f.be = s[S_BETA];
        f.cont = s[S_DONE] == 0.0;
    }
    return f;
}
template <bool FOLD>
__device__ inline void cg_beta_commit(double* s, const FoldBeta& f, bool first_block) {
    if constexpr (FOLD) {
        if (first_block && threadIdx.x == 0) {
            const double rrn = s[S_RRNEW];
            s[S_BETA] = f.be;
            s[S_RR] = rrn;
            s[S_ITERS] += 1.0;
            if (!f.cont) s[S_DONE] = 1.0;
        }
    }
}
// PACK (partitioned lattice, halo_fuse bit 1): the FIRST npk blocks of the launch are pack blocks (dispatched first: the faces are what the next
// launch on the critical path waits for) -- they form p' = r + beta p at the face sites in registers and write the send buffers of the next
// D p (stencil_common.h wilson_pack_axpy_block), so that application needs no pack launch; the other nbf blocks do the flat update.
template <bool NT, bool FOLD, bool PACK = false>      // NT: streaming (non-temporal) loads and stores for fields that are not re-used before they fall out of every cache
__global__ __launch_bounds__(UB) void cg_update_even(double* __restrict__ s, double2* __restrict__ x, const double2* __restrict__ pk,
                                                      double2* __restrict__ pnext, const double2* __restrict__ r, size_t n, int nbf, HArgs h, int npx) {
    if (s[S_XDONE] != 0.0) return;
    const FoldBeta fb = cg_beta<FOLD>(s);
    const double al = s[S_ALPHA], be = fb.be;
    const bool cont = fb.cont;
    const int npk = PACK ? 8 * npx : 0, fb0 = (int)blockIdx.x - npk;      // fb0: index among the flat blocks
    if constexpr (PACK) {
        if (fb0 < 0) {
            if (cont) wilson_pack_axpy_block(h, (int)blockIdx.x, npx, be);
            return;
        }
    }
    if (cont) {
        for (size_t i = (size_t)fb0 * UB + threadIdx.x; i < n; i += (size_t)nbf * UB) {
            const double2 pv = ldx<NT>(pk + i), rv = ldx<NT>(r + i);
            double2 o;
            o.x = fma(be, pv.x, rv.x); o.y = fma(be, pv.y, rv.y);
            stx<NT>(pnext + i, o);
        }
        if (fb0 == 0 && threadIdx.x == 0) s[S_APREV] = al;
    } else {
        for (size_t i = (size_t)fb0 * UB + threadIdx.x; i < n; i += (size_t)nbf * UB) {
            const double2 pv = pk[i];
            double2 xv = x[i];
            xv.x = fma(al, pv.x, xv.x); xv.y = fma(al, pv.y, xv.y);
            x[i] = xv;
        }
    }
    cg_beta_commit<FOLD>(s, fb, fb0 == 0);
}
template <bool NT, bool FOLD, bool PACK = false>
__global__ __launch_bounds__(UB) void cg_update_odd(double* __restrict__ s, double2* __restrict__ x, double2* __restrict__ pprev,
                                                     const double2* __restrict__ pk, const double2* __restrict__ r, size_t n, int nbf, HArgs h, int npx) {
    if (s[S_XDONE] != 0.0) return;
    const FoldBeta fb = cg_beta<FOLD>(s);
    const double ap = s[S_APREV], al = s[S_ALPHA], be = fb.be;
    const bool cont = fb.cont;
    const int npk = PACK ? 8 * npx : 0, fb0 = (int)blockIdx.x - npk;
    if constexpr (PACK) {
        if (fb0 < 0) {
            if (cont) wilson_pack_axpy_block(h, (int)blockIdx.x, npx, be);
            return;
        }
    }
    for (size_t i = (size_t)fb0 * UB + threadIdx.x; i < n; i += (size_t)nbf * UB) {
        const double2 pp = ldx<NT>(pprev + i), pv = ldx<NT>(pk + i);
        double2 xv = ldx<NT>(x + i);
        xv.x = fma(ap, pp.x, xv.x); xv.y = fma(ap, pp.y, xv.y);
        xv.x = fma(al, pv.x, xv.x); xv.y = fma(al, pv.y, xv.y);
        stx<NT>(x + i, xv);
        if (cont) {
            const double2 rv = ldx<NT>(r + i);
            double2 o;
            o.x = fma(be, pv.x, rv.x); o.y = fma(be, pv.y, rv.y);
            stx<NT>(pprev + i, o);
        }
    }
    cg_beta_commit<FOLD>(s, fb, fb0 == 0);
}
// x += alpha_k p_k for a window that ended (unconverged) on an even iteration
__global__ __launch_bounds__(UB) void cg_flush_kernel(const double* __restrict__ s, double2* __restrict__ x, const double2* __restrict__ pk, size_t n) {
    if (s[S_DONE] != 0.0) return;
    const double ap = s[S_APREV];
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        const double2 pv = pk[i];
        double2 xv = x[i];
        xv.x = fma(ap, pv.x, xv.x); xv.y = fma(ap, pv.y, xv.y);
        x[i] = xv;
    }
}
// Deferred x update over a ring of K search-direction buffers (cg_defer_x = K >= 3): p_k lives in buffer k % K.  Iteration k with m = k % K < K - 1:
// p_{k+1} = r + beta p_k into the next buffer, alpha_k kept in S_AHIST[m], x untouched -- 3 streams.  m = K - 1 (or the iteration that converges, whatever m):
// x += alpha_{k-m} p_{k-m} + ... + alpha_k p_k in that order (the operations two single updates would do: identical bits), then p_{k+1} over the oldest buffer,
// which this thread has just read -- K + 4 streams.  (4 K + 1) / K passes per iteration instead of the 4.5 of the two-buffer form.
struct CgRing { const double2* b[8]; };      // the buffers that hold pending directions, oldest first (entries >= m unused); indexed by unrolled constants only
template <bool NT, bool FOLD, bool PACK = false>
__global__ __launch_bounds__(UB) void cg_update_ring(double* __restrict__ s, double2* __restrict__ x, CgRing ring, int m, int flush, const double2* __restrict__ pk,
                                                      double2* pnext, const double2* __restrict__ r, size_t n, int nbf, HArgs h, int npx) {
    if (s[S_XDONE] != 0.0) return;
    const FoldBeta fb = cg_beta<FOLD>(s);
    const double al = s[S_ALPHA], be = fb.be;
    const bool cont = fb.cont;
    const int npk = PACK ? 8 * npx : 0, fb0 = (int)blockIdx.x - npk;
    if constexpr (PACK) {
        if (fb0 < 0) {
            if (cont) wilson_pack_axpy_block(h, (int)blockIdx.x, npx, be);
            return;
        }
    }
    if (flush || !cont) {
        double ah[8];
#pragma unroll
        for (int j = 0; j < 8; j++) ah[j] = j < m ? s[S_AHIST + j] : 0.0;
        for (size_t i = (size_t)fb0 * UB + threadIdx.x; i < n; i += (size_t)nbf * UB) {
            double2 xv = ldx<NT>(x + i);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (j < m) {
                    const double2 pj = ldx<NT>(ring.b[j] + i);
                    xv.x = fma(ah[j], pj.x, xv.x); xv.y = fma(ah[j], pj.y, xv.y);
                }
            }
            const double2 pv = ldx<NT>(pk + i);
            xv.x = fma(al, pv.x, xv.x); xv.y = fma(al, pv.y, xv.y);
            stx<NT>(x + i, xv);
            if (cont) {
                const double2 rv = ldx<NT>(r + i);
                double2 o;
                o.x = fma(be, pv.x, rv.x); o.y = fma(be, pv.y, rv.y);
                stx<NT>(pnext + i, o);
            }
        }
    } else {
        for (size_t i = (size_t)fb0 * UB + threadIdx.x; i < n; i += (size_t)nbf * UB) {
            const double2 pv = ldx<NT>(pk + i), rv = ldx<NT>(r + i);
            double2 o;
            o.x = fma(be, pv.x, rv.x); o.y = fma(be, pv.y, rv.y);
            stx<NT>(pnext + i, o);
        }
        if (fb0 == 0 && threadIdx.x == 0) s[S_AHIST + m] = al;
    }
    cg_beta_commit<FOLD>(s, fb, fb0 == 0);
}
// x += sum of the m pending terms, for a window that ended (unconverged) in the middle of the ring
__global__ __launch_bounds__(UB) void cg_flush_ring(const double* __restrict__ s, double2* __restrict__ x, CgRing ring, int m, size_t n) {
    if (s[S_DONE] != 0.0) return;
    double ah[8];
#pragma unroll
    for (int j = 0; j < 8; j++) ah[j] = j < m ? s[S_AHIST + j] : 0.0;
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        double2 xv = x[i];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (j < m) {
                const double2 pj = ring.b[j][i];
                xv.x = fma(ah[j], pj.x, xv.x); xv.y = fma(ah[j], pj.y, xv.y);
            }
        }
        x[i] = xv;
    }
}
// ---- cg_fused = 3, the residual ring: D p by recurrence from D r; p and x brought up to date once per K iterations (tunable cg_rring = K = 2, 4, 8; with the tunable
// cg_rring_mult = M = 2, 4 the ring has K M <= 32 slots and everything below holds with K M in place of K -- the depth; cg_rring_active reports K, cg_rring_depth_active K M).
// With s_k = D p_k and p_{k+1} = r_{k+1} + beta_k p_k:  s_{k+1} = D r_{k+1} + beta_k s_k.  The stencil is applied to the residual the D^+ before it has just written
// (recurrence mode of the scalar-addressing kernel: s read at the centre, s = v + beta s stored in place), so p is needed only to accumulate x: the K residuals of a
// batch stay in a ring of K slots (update-mode D^+ reads r_k from slot k % K and writes r_{k+1} to the next), alpha_k / beta_k go to S_AHIST / S_BHIST, and every K-th
// iteration ONE streaming launch (cg_batch_px) forms x and p by the fma sequence of cg_update_xp; the D behind it is a plain D on the fresh p, which restarts the
// recurrence (its rounding error lives for at most K - 1 steps).  Per site and iteration: 864 B (D, recurrence mode) + 864 B (D^+) + ((K + 4) 192 + 672 - 864) / K B
// = 2208 / 2064 / 1992 / 1944 / 1920 B for depth 2 / 4 / 8 / 16 / 32, against the 2400 B of the two-buffer deferred-x form; 4 + 1 / K launches instead of 5.  The batch
// kernel alone: 192 (K + 4) / K = 288 / 240 / 216 B per site and iteration at depth 8 / 16 / 32; 192 of them are the one further read of each residual.
// Where: cg_setup's gate (cg_rring_wanted) -- Wilson, r = 1, no clover term, one unpartitioned GPU without a communicator, the scalar-addressing kernel, beyond cg_small.
// Costed and not built: (a) the batch folded into the D behind it -- the stencil would read the K residuals and p at every NEIGHBOUR as well (the new p is its
// hop operand): 8 x (K + 1) more reads than the K + 4 streams it saves; (b) a depth that neither divides 8 nor is a multiple of it -- a captured burst bakes the slot
// roles in, the replay must find the ring where it left it (cg_run captures max(8, K M) iterations); (c) staggered, fp32 / mixed-precision, multi-shift, even-odd and partitioned solvers: the same recurrence applies, their
// kernels have no centre read separate from the store ("not done").
struct CgSlots { const double2* r[RRING_MAX]; };      // slot of r_{b+j+1}, j = 0..depth-1, b the first iteration of the batch (entries >= depth unused); indexed by unrolled constants only
// x += alpha_j p_j, p_{j+1} = r_{j+1} + beta_j p_j for the pending iterations j = 0 .. np - 1, oldest first (np = S_ITERS - S_BSTART, from the device).  fin = 0 (batch
// boundary inside a window): np = DEPTH, writes x and p; a no-op once the solve is done.  fin = 1 (cg_flush_x: a converged solve, an exhausted one, the end of a window):
// applies the np pending terms to x, whatever the done flag says, and forms no p nobody uses.  One instance per ring depth (8: cg_rring = 2, 4, 8 with cg_rring_mult = 1;
// 16, 32), the loop over the pending iterations fully unrolled; one pass per element: x, p and the slots are read once, x and p written once.  At DEPTH 32 the full
// batch (fin = 0, np = DEPTH) takes a loop without a test on np, so the 34 loads of an element are independent of every branch and the compiler issues them together
// (164 VGPRs, three waves per SIMD); the fma sequence per element is the same on both paths.  Measured (profiles/r17_rring_depth_ab.log): that loop is +1.1 % on the
// iteration at depth 32, nothing at 16 and -1.6 % at 8 -- so depths 8 and 16 keep the plain loop alone (20 / 22 VGPRs), and depth 8 is the kernel it always was.
template <bool NT, int DEPTH>
__global__ __launch_bounds__(UB) void cg_batch_px(const double* __restrict__ s, double2* __restrict__ x, double2* __restrict__ p, CgSlots sl, int fin, size_t n) {
    const int np = (int)(s[S_ITERS] - s[S_BSTART]);
    if (np <= 0 || np > DEPTH || (!fin && s[S_DONE] != 0.0)) return;
    double al[DEPTH], be[DEPTH];
#pragma unroll
    for (int j = 0; j < DEPTH; j++) { al[j] = j < np ? s[S_AHIST + j] : 0.0; be[j] = j < np ? s[S_BHIST + j] : 0.0; }
    if (DEPTH >= 32 && !fin && np == DEPTH) {
        for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
            double2 xv = ldx<NT>(x + i), pv = ldx<NT>(p + i);
            double2 rv[DEPTH];
#pragma unroll
            for (int j = 0; j < DEPTH; j++) rv[j] = ldx<NT>(sl.r[j] + i);
#pragma unroll
            for (int j = 0; j < DEPTH; j++) {
                xv.x = fma(al[j], pv.x, xv.x); xv.y = fma(al[j], pv.y, xv.y);
                pv.x = fma(be[j], pv.x, rv[j].x); pv.y = fma(be[j], pv.y, rv[j].y);
            }
            stx<NT>(x + i, xv);
            stx<NT>(p + i, pv);
        }
        return;
    }
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        double2 xv = ldx<NT>(x + i), pv = ldx<NT>(p + i);
#pragma unroll
        for (int j = 0; j < DEPTH; j++) {
            if (j < np) {
                xv.x = fma(al[j], pv.x, xv.x); xv.y = fma(al[j], pv.y, xv.y);
                if (!fin || j < np - 1) {
                    const double2 rv = ldx<NT>(sl.r[j] + i);
                    pv.x = fma(be[j], pv.x, rv.x); pv.y = fma(be[j], pv.y, rv.y);
                }
            }
        }
        stx<NT>(x + i, xv);
        if (!fin) stx<NT>(p + i, pv);
    }
}
// p = r + beta p
__global__ __launch_bounds__(UB) void cg_update_p(const double* __restrict__ s, double2* __restrict__ p, const double2* __restrict__ r, size_t n) {
    if (s[S_DONE] != 0.0) return;
    const double be = s[S_BETA];
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        const double2 rv = r[i];
        double2 pv = p[i];
        pv.x = fma(be, pv.x, rv.x); pv.y = fma(be, pv.y, rv.y);
        p[i] = pv;
    }
}
__global__ __launch_bounds__(UB) void norm2_partial_kernel(const double2* __restrict__ a, size_t n, double* partial) {
    __shared__ double red[UB / 64];
    double acc = 0;
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        const double2 v = a[i];
        acc = fma(v.x, v.x, acc); acc = fma(v.y, v.y, acc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0;
        for (int w = 0; w < UB / 64; w++) t += red[w];
        partial[blockIdx.x] = t;
    }
}
// re(p.q) partials (unfused reference form c1 = p.q)
__global__ __launch_bounds__(UB) void redot_partial_kernel(const double2* __restrict__ a, const double2* __restrict__ b, size_t n, double* partial) {
    __shared__ double red[UB / 64];
    double acc = 0;
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        const double2 x = a[i], y = b[i];
        acc = fma(x.x, y.x, acc); acc = fma(x.y, y.y, acc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0;
        for (int w = 0; w < UB / 64; w++) t += red[w];
        partial[blockIdx.x] = t;
    }
}


// ---------------------------------------------------------------------------------- temporal gauge (fields.hip gauge_ensure_tgauge)
// psi <- G psi / G^+ psi, colour rotation of a full Wilson field by the gauge-transformation field: one site per thread, [chunk][component][lane] rows of 1 KiB,
// su3_mv's fma order.  dst may be src.
template <bool ADJ>
__global__ __launch_bounds__(UB) void spinor_gauge_rotate_kernel(Geom g, const double2* __restrict__ gf, double2* dst, const double2* src) {
    const int i = blockIdx.x * UB + threadIdx.x, p = blockIdx.y;
    if (i >= g.Vh) return;
    const size_t so = (size_t)p * 12 * g.Vs + sp_off(12, i);
    const int Ss = sp_stride(g);
    cd G[9], in[12], out[12];
    const double2* gp = gf + gfix_off(g, p, i);
#pragma unroll
    for (int e = 0; e < 9; e++) G[e] = ld(gp + (size_t)e * 64);
#pragma unroll
    for (int j = 0; j < 12; j++) in[j] = ld(src + so + (size_t)j * Ss);
#pragma unroll
    for (int sp = 0; sp < 4; sp++) {
        cd h[3] = {in[3 * sp], in[3 * sp + 1], in[3 * sp + 2]}, chi[3];
        su3_mv<ADJ>(chi, G, h);
#pragma unroll
        for (int cc = 0; cc < 3; cc++) out[3 * sp + cc] = chi[cc];
    }
#pragma unroll
    for (int j = 0; j < 12; j++) st(dst + so + (size_t)j * Ss, out[j]);
}
int spinor_gauge_rotate(lqcd_ctx_s* c, const double2* gfix, double2* dst, const double2* src, int adjoint) {
    const dim3 grid((c->geom.Vh + UB - 1) / UB, 2), block(UB);
    if (adjoint) hipLaunchKernelGGL((spinor_gauge_rotate_kernel<true>), grid, block, 0, c->stream, c->geom, gfix, dst, src);
    else hipLaunchKernelGGL((spinor_gauge_rotate_kernel<false>), grid, block, 0, c->stream, c->geom, gfix, dst, src);
    HIPCHK(hipGetLastError());
    return LQCD_OK;
}

// cg_small applies when the reductions are local (no communicator), at most 1024 block partials exist, and the stencil kernel in use
// takes alpha from emit()'s argument (every variant but the hop-split ones)
static bool cg_small_ok(lqcd_op_s* op, int nbs) {
    lqcd_ctx_s* c = op->ctx;
    if (any_partitioned(c) || c->has_comm || nbs > 1024) return false;
    const int v = c->tun.dslash_variant;
#ifdef LQCD_VARIANTS
    if (op->kind == LQCD_WILSON && op->r == 1.0 && (v == 2 || v == 3)) return false;
#endif
    (void)v;
    if ((c->tun.dslash_pipe == 1 || c->tun.dslash_pipe == 3) && wilson_pipe_applies(c, op->kind, op->r, 2, op_fused_clover(op))) return false;    // pipelined kernels: no alpha_partials form
    return true;
}

int cg_work_get(lqcd_ctx_s* c, int kind, CgWork& w) {
    w.r = scratch_get(c, kind, LQCD_FULL); w.p = scratch_get(c, kind, LQCD_FULL);
    w.q = scratch_get(c, kind, LQCD_FULL); w.tmp = scratch_get(c, kind, LQCD_FULL);
    if (!(w.r && w.p && w.q && w.tmp)) { cg_work_put(w); return LQCD_ERR_HIP; }
    return LQCD_OK;
}
void cg_work_put(CgWork& w) {
    for (lqcd_spinor_s** f : {&w.r, &w.p, &w.q, &w.tmp}) { if (*f) scratch_put(*f); *f = nullptr; }
    for (lqcd_spinor_s*& f : w.more) { if (f) scratch_put(f); f = nullptr; }
}
// buffers of the deferred-x form: 2, or the ring of cg_defer_x = K = 3..8 (cg_setup takes the extra ones from the scratch pool; if the pool cannot grow: 2)
// Measured (profiles/r05_cg_ring.log): at 32^3x64 on one GPU the ring does not pay (K = 2 / 4 / 8: 919.8 / 912.6 / 913.5 iter/s -- the flush kernel's K + 4 streams cost what
// the saved passes win); at the N = 8 local volume, where the vectors live in the Infinity Cache, it does (5207 / 5254 / 5286 iter/s).  cg_defer_x = 1 (default) therefore
// means: two buffers on an unpartitioned lattice, a ring of 8 on a partitioned one; 2 and 3..8 force a size.
static int cg_ring_wanted(lqcd_op_s* op) {
    const int k = op->ctx->tun.cg_defer_x;
    if (op->kind == LQCD_DOMAINWALL) return 2;
    if (k >= 3) return std::min(k, 8);
    return (k == 1 && any_partitioned(op->ctx)) ? 8 : 2;
}
static CgRing cg_ring_pending(const CgWork& w, int m) {      // the buffers of p_{k-m} .. p_{k-1}, oldest first, for k = w.k
    CgRing ring;
    for (int j = 0; j < 8; j++) ring.b[j] = j < m ? w.buf((w.k - m + j) % w.ring)->data : nullptr;
    return ring;
}
template <int DEPTH>
static void cg_batch_launch_depth(lqcd_ctx_s* c, bool nt, dim3 g, dim3 b, lqcd_spinor_s* x, CgWork& w, const CgSlots& sl, int fin) {
    if (nt) hipLaunchKernelGGL((cg_batch_px<true, DEPTH>), g, b, 0, c->stream, c->d_scal, x->data, w.p->data, sl, fin, x->elems);
    else hipLaunchKernelGGL((cg_batch_px<false, DEPTH>), g, b, 0, c->stream, c->d_scal, x->data, w.p->data, sl, fin, x->elems);
}
static int cg_batch_launch(lqcd_ctx_s* c, lqcd_spinor_s* x, CgWork& w, int fin) {
    CgSlots sl;
    for (int j = 0; j < RRING_MAX; j++) sl.r[j] = j < w.rring ? w.slot((j + 1) % w.rring)->data : nullptr;
    const dim3 g(stream_grid(c, x->elems)), b(UB);
    const bool nt = c->tun.nt_blas != 0;
    if (w.rring <= 8) cg_batch_launch_depth<8>(c, nt, g, b, x, w, sl, fin);
    else if (w.rring == 16) cg_batch_launch_depth<16>(c, nt, g, b, x, w, sl, fin);
    else cg_batch_launch_depth<32>(c, nt, g, b, x, w, sl, fin);
    HIPCHK(hipGetLastError());
    return LQCD_OK;
}
int cg_flush_x(lqcd_op_s* op, lqcd_spinor_s* x, CgWork& w) {
    lqcd_ctx_s* c = op->ctx;
    if (w.form == CgForm::RRing) {      // residual ring: the pending terms of the open batch (also behind the converging iteration: no launch of the iteration updates x)
        if (w.flushed || w.k == 0) return LQCD_OK;
        w.flushed = true;      // (a window is never continued after its flush)
        return cg_batch_launch(c, x, w, 1);
    }
    const bool deferred = w.form == CgForm::DeferX;
    if (deferred && w.ring > 2) {
        const int m = w.k % w.ring;       // directions p_{k-m} .. p_{k-1} are still to be added
        if (m == 0) return LQCD_OK;
        hipLaunchKernelGGL(cg_flush_ring, dim3(stream_grid(c, x->elems)), dim3(UB), 0, c->stream, c->d_scal, x->data, cg_ring_pending(w, m), m, x->elems);
        HIPCHK(hipGetLastError());
        w.k += w.ring - m;      // nothing pending any more (a window is never continued after its flush)
        return LQCD_OK;
    }
    if (!deferred || !(w.k & 1)) return LQCD_OK;
    const size_t n = x->elems;
    hipLaunchKernelGGL(cg_flush_kernel, dim3(stream_grid(c, n)), dim3(UB), 0, c->stream, c->d_scal, x->data, w.p->data, n);   // p_k of an even k lives in w.p
    HIPCHK(hipGetLastError());
    w.k++;      // nothing pending any more (a window is never continued after its flush)
    return LQCD_OK;
}

int cg_finish(lqcd_op_s* op, lqcd_spinor_s* x, CgWork& w, bool flush) {
    int st = flush ? cg_flush_x(op, x, w) : LQCD_OK;
    if (w.tgauge) {      // (also behind a failed flush: the caller's x leaves the rotated basis on every path)
        const int sr = spinor_gauge_rotate(op->ctx, w.gfix, x->data, x->data, 1);
        if (st == LQCD_OK) st = sr;
        w.tgauge = false;
    }
    return st;
}
bool cg_gauge_moved(lqcd_op_s* op, const CgWork& w) {
    return w.tgauge && (op->gauge->version != w.gauge_version || op->gauge->data12t != w.links_t || (w.links_t8 && op->gauge->data8t != w.links_t8));
}

// The solve runs in temporal gauge when: Wilson, r = 1, no clover term, unpartitioned lattice, the stencil launches of the iteration take the TG instances
// (asked before anything is rotated), the rotated copy of this version of the links passed its gate, and the tunable cg_tgauge allows it -- 1: beyond the
// cg_small regime only (below it an iteration is launch latency and the three rotations of a solve are pure cost), 2: whenever admissible.
static bool cg_tgauge_wanted(lqcd_op_s* op) {
    lqcd_ctx_s* c = op->ctx;
    if (!c->tun.cg_tgauge || op->kind != LQCD_WILSON || op->r != 1.0 || op->csw != 0.0 || any_partitioned(c) || !c->local_peers.empty()) return false;
    if (!stencil_tgauge_applies(c, op->kind, op->r, op_fused_clover(op))) return false;
    if (c->tun.cg_tgauge < 2 && stencil_num_partials(c, op->kind, op->r, 2, 0, op_fused_clover(op)) <= 1024) return false;
    return gauge_ensure_tgauge(op->gauge) == LQCD_OK && op->gauge->tgauge_ok;
}

// one iteration of the residual-ring form (see cg_batch_px): k % K = 0: batch kernel (nothing pending at k = 0: a no-op that keeps a captured burst replayable), plain D on p;
// otherwise D in recurrence mode on r_k.  Then alpha (+ history), D^+ from slot k % K into the next, beta (+ history, convergence).  No update launch.
static int cg_enqueue_rring(lqcd_op_s* op, lqcd_spinor_s* x, CgWork& w) {
    lqcd_ctx_s* c = op->ctx;
    if (w.flushed) { set_error("CG: the window was flushed; it cannot be continued"); return LQCD_ERR_ARG; }
    const double2* gt = w.tgauge ? w.links_t : nullptr;
    const int K = w.rring, m = w.k % K;
    const int nbs = stencil_num_partials(c, op->kind, op->r, 2, 0, op_fused_clover(op));
    lqcd_spinor_s *rk = w.slot(m), *rn = w.slot((m + 1) % K);
    StencilCall s1;
    if (m == 0) {
        LQCHK(cg_batch_launch(c, x, w, 0));
        apply_bc(c, op->bc);
        LQCHK(make_full_call(op, w.tmp, w.p, 0, s1));
        s1.skip_flag = c->tun.cg_skip_done ? c->d_scal : nullptr;
    } else {
        apply_bc(c, op->bc);
        LQCHK(make_full_call(op, w.tmp, rk, 0, s1));
        s1.upd_scal = c->d_scal;      // (its done flag is the mandatory one: the store is in place)
        s1.upd[0] = spinor_block(w.tmp, 0);
        s1.upd[1] = spinor_block(w.tmp, 1);
        s1.upd_rec = 1;
    }
    s1.gauge12t = gt;
    s1.gauge8t = w.links_t8;
    s1.keep_slabs = w.store_keep;            // (-1 unless the sweep alternates: the slabs D^+ starts on store plain, the others stream)
    s1.norm_partial = c->d_partial;
    LQCHK(stencil_apply(c, s1));
    LQCHK(reduce_to_slot(c, nbs, 1, S_PQ, true, m == 0 ? 9 : 7));      // + alpha = rr / |s|^2 into the history (9: a batch opens)
    apply_bc(c, op->bc);
    StencilCall s2;
    LQCHK(make_full_call(op, rn, w.tmp, 1, s2));
    s2.gauge12t = gt;
    s2.gauge8t = w.links_t8;
    s2.sweep_rev = w.sweep_alt ? 1 : 0;      // D^+ backwards: it starts on the slabs the D above wrote last, the next D starts on the slabs it writes last
    s2.keep_slabs = w.store_keep;            // ... and only those store r_{k+1} plain
    s2.norm_partial = c->d_partial;
    s2.upd_scal = c->d_scal;
    for (int q = 0; q < 2; q++) { s2.upd[q] = spinor_block(rn, q); s2.upd_src[q] = spinor_block(rk, q); }
    LQCHK(stencil_apply(c, s2));
    LQCHK(reduce_to_slot(c, nbs, 1, S_RRNEW, true, 8));               // + beta into the history, convergence flag
    w.k++;
    return LQCD_OK;
}
// the residual ring applies: Wilson, r = 1, no clover term, one unpartitioned GPU without a communicator, every stencil launch of the iteration takes the
// scalar-addressing kernel (12-real, 18-real, 12 + delta or temporal-gauge instance).  Returns K (tunable cg_rring), 0 if not.  Asked by cg_setup behind the cg_small test.
static int cg_rring_wanted(lqcd_op_s* op, const CgWork& w) {
    lqcd_ctx_s* c = op->ctx;
    const int K = c->tun.cg_rring;
    if (c->tun.cg_fused < 3 || !(K == 2 || K == 4 || K == 8)) return 0;
    if (op->kind != LQCD_WILSON || op->r != 1.0 || op->csw != 0.0 || any_partitioned(c) || c->has_comm || !c->local_peers.empty()) return 0;
    if (!stencil_sdir_applies(c, op->kind, op->r, op_fused_clover(op))) return 0;
    StencilCall s;      // the links this operator's calls read: the 18 stored reals take the kernel only with dslash_s18
    if (make_full_call(op, w.tmp, w.p, 0, s) != LQCD_OK) return 0;
    if (!(w.tgauge || s.gauge12 || c->tun.dslash_s18)) return 0;
    return K;
}

// ---- the iteration forms (CgWork::form, chosen by cg_setup): each enqueues one CG iteration on the compute stream, no host synchronisation

// the streaming tail of the Reference / NormFused forms and of cg_generic, on raw buffers: [S_PQ = re(p . q) ;] alpha ; x += alpha p, r -= alpha q, |r|^2 ; beta,
// convergence ; p = r + beta p
static int cg_plain_tail(lqcd_ctx_s* c, double2* x, double2* r, double2* p, const double2* q, size_t n, bool dot_pq) {
    const int nb = stream_grid(c, n);
    if (dot_pq) {
        hipLaunchKernelGGL(redot_partial_kernel, dim3(nb), dim3(UB), 0, c->stream, p, q, n, c->d_partial);
        HIPCHK(hipGetLastError());
        LQCHK(reduce_to_slot(c, nb, 1, S_PQ, true));
    }
    hipLaunchKernelGGL(cg_scalar_alpha, dim3(1), dim3(1), 0, c->stream, c->d_scal);
    hipLaunchKernelGGL(cg_update_xr, dim3(nb), dim3(UB), 0, c->stream, c->d_scal, x, r, p, q, n, c->d_partial);
    HIPCHK(hipGetLastError());
    LQCHK(reduce_to_slot(c, nb, 1, S_RRNEW, true));
    hipLaunchKernelGGL(cg_scalar_beta, dim3(1), dim3(1), 0, c->stream, c->d_scal);
    hipLaunchKernelGGL(cg_update_p, dim3(nb), dim3(UB), 0, c->stream, c->d_scal, p, r, n);
    HIPCHK(hipGetLastError());
    return LQCD_OK;
}
// Reference: c1 = p . q with q = D^+ D p.  NormFused: c1 = |D p|^2, its block partials fused into the stencil when the lattice is not partitioned.
static int cg_iter_reference(lqcd_op_s* op, lqcd_spinor_s* x, CgWork& w) {
    lqcd_ctx_s* c = op->ctx;
    const size_t n = x->elems;
    const double2* gt = w.tgauge ? w.links_t : nullptr;      // temporal gauge: every stencil call reads the rotated links
    const bool norm = w.form == CgForm::NormFused, fuse = norm && !any_partitioned(c);
    LQCHK(op_apply_async(op, w.tmp, w.p, 0, fuse ? c->d_partial : nullptr, nullptr, gt));      // tmp = D p
    if (fuse) {
        LQCHK(reduce_to_slot(c, stencil_num_blocks(c, op->kind, op->r, 2, 0, op_fused_clover(op)), 1, S_PQ, true));
    } else if (norm) {
        const int nb = stream_grid(c, n);
        hipLaunchKernelGGL(norm2_partial_kernel, dim3(nb), dim3(UB), 0, c->stream, w.tmp->data, n, c->d_partial);
        HIPCHK(hipGetLastError());
        LQCHK(reduce_to_slot(c, nb, 1, S_PQ, true));
    }
    LQCHK(op_apply_async(op, w.q, w.tmp, 1, nullptr, nullptr, gt));
    return cg_plain_tail(c, x->data, w.r->data, w.p->data, w.q->data, n, !norm);
}
// Small lattices: launch latency is the cost.  Same arithmetic as the fused form below, but the two single-block reductions
// are folded into the prologues of their consumers -- 3 dependent launches per iteration instead of 5, identical iterates.
static int cg_iter_small(lqcd_op_s* op, lqcd_spinor_s* x, CgWork& w) {
    lqcd_ctx_s* c = op->ctx;
    const size_t n = x->elems;
    const double2* gt = w.tgauge ? w.links_t : nullptr;
    const int nbs_small = stencil_num_partials(c, op->kind, op->r, 2, 0, op_fused_clover(op));
    double* part_a = c->d_partial;            // |D p|^2 block partials
    double* part_b = c->d_partial + 2048;     // |r|^2 block partials (the update-mode kernel reads part_a while its blocks write these)
    LQCHK(op_apply_async(op, w.tmp, w.p, 0, part_a, c->tun.cg_skip_done ? c->d_scal : nullptr, gt));
    apply_bc(c, op->bc);
    StencilCall s2;
    LQCHK(make_full_call(op, w.q, w.tmp, 1, s2));
    s2.gauge12t = gt;
    s2.norm_partial = part_b;
    s2.upd_scal = c->d_scal;
    s2.upd[0] = spinor_block(w.r, 0);
    s2.upd[1] = spinor_block(w.r, 1);
    s2.alpha_partials = part_a; s2.alpha_n = nbs_small; s2.scal_w = c->d_scal;
    LQCHK(stencil_apply(c, s2));
    const int nbu = stream_grid(c, n);
    hipLaunchKernelGGL(cg_update_xp_small, dim3(nbu), dim3(UB), 0, c->stream, c->d_scal, x->data, w.p->data, w.r->data, n, part_b, nbs_small);
    HIPCHK(hipGetLastError());
    return LQCD_OK;
}
// the x / p update launch of the DeferX form, instance <NT, FOLD, PACK> of cg_update_ring (ring > 2) or, by the parity of k, cg_update_odd / cg_update_even
struct CgUpd { dim3 grid; double2 *x, *pk, *po; size_t n; int nbu; HArgs h; int npx; };
template <bool NT, bool FOLD, bool PACK>
static void cg_launch_update_defer(lqcd_ctx_s* c, const CgWork& w, const CgUpd& u) {
    const dim3 ub(UB);
    if (w.ring > 2) {
        const int rm = w.k % w.ring, rflush = rm == w.ring - 1 ? 1 : 0;
        hipLaunchKernelGGL((cg_update_ring<NT, FOLD, PACK>), u.grid, ub, 0, c->stream, c->d_scal, u.x, cg_ring_pending(w, rm), rm, rflush, u.pk, u.po, w.r->data, u.n, u.nbu, u.h, u.npx);
    }
    else if (w.k & 1) hipLaunchKernelGGL((cg_update_odd<NT, FOLD, PACK>), u.grid, ub, 0, c->stream, c->d_scal, u.x, u.po, u.pk, w.r->data, u.n, u.nbu, u.h, u.npx);
    else hipLaunchKernelGGL((cg_update_even<NT, FOLD, PACK>), u.grid, ub, 0, c->stream, c->d_scal, u.x, u.pk, u.po, w.r->data, u.n, u.nbu, u.h, u.npx);
}
// Fused and DeferX: 10 spinor passes per iteration instead of 13, q = D^+ D p is never written
//   tmp = D p [+ |tmp|^2 partials] ; alpha = rr / |tmp|^2 ; D^+ tmp with epilogue r -= alpha q [+ |r|^2 partials] ;
//   beta, convergence ; x += alpha p, p = r + beta p
static int cg_iter_fused(lqcd_op_s* op, lqcd_spinor_s* x, CgWork& w) {
    lqcd_ctx_s* c = op->ctx;
    const size_t n = x->elems;
    const double2* gt = w.tgauge ? w.links_t : nullptr;
    const int nbs = stencil_num_partials(c, op->kind, op->r, 2, 0, op_fused_clover(op));
    const bool defer = w.form == CgForm::DeferX;
    const bool ringed = defer && w.ring > 2;
    lqcd_spinor_s* pk = ringed ? w.buf(w.k % w.ring) : (defer && (w.k & 1)) ? w.q : w.p;        // q = D^+D p is never written in this form: its buffer is the second p
    lqcd_spinor_s* po = ringed ? w.buf((w.k + 1) % w.ring) : (defer && (w.k & 1)) ? w.p : w.q;
    // several ranks: reduce_final -> all-reduce -> one-thread scalar kernel are three dependent launches per reduction; with `fold` the scalar
    // steps move into the prologues of the kernels that consume them (deferred-x form only)
    const bool fold = c->has_comm && defer && c->tun.cg_fold_scalars;
    // partitioned lattice (RCCL path): at small local volumes the iteration is a chain of short dependent launches.  halo_fuse bit 0: the
    // exterior kernel's last block sums the |.|^2 partials (no reduce_final launch); bit 1: the exterior of D p packs the faces of
    // tmp = D p for the D^+ that follows and the x/p update packs the new search direction for the next D p (no pack launches).
    // Wilson r = 1 only (a general-r application is two r = 1 passes with different projectors).
    const bool part = any_partitioned(c) && c->has_comm && c->local_peers.empty();
    const bool folded = part && halo_fold_applies(c, op->kind, op->r, 2, 0, op_fused_clover(op));      // no exterior launch: nothing for bit 0 to ride on
    const bool fr = part && (c->tun.halo_fuse & 1) && !folded;
    const bool fp = part && defer && (c->tun.halo_fuse & 2) && op->kind == LQCD_WILSON && op->r == 1.0;
    {
        apply_bc(c, op->bc);      // another operator of this context (other boundary signs) may have been applied since the last iteration of an open session
        StencilCall s1;
        LQCHK(make_full_call(op, w.tmp, pk, 0, s1));
        s1.gauge12t = gt;
        s1.gauge8t = w.links_t8;
        s1.keep_slabs = w.store_keep;      // (see cg_enqueue_rring)
        s1.norm_partial = c->d_partial;
        s1.skip_flag = c->tun.cg_skip_done ? c->d_scal : nullptr;      // a no-op once the solve has converged inside a burst
        if (fr) s1.red_slot = S_PQ;
        if (fp) { s1.pack_next = 1; s1.prepacked = (w.p_packed && w.pack_epoch == c->halo_epoch) ? 1 : 0; s1.defer_pack = folded ? 1 : 0; }
        LQCHK(stencil_apply(c, s1));
    }
    LQCHK(fr ? reduce_tail(c, 1, S_PQ, fold ? 0 : 1) : reduce_pack_to_slot(c, nbs, S_PQ, fold ? 0 : 1));      // + alpha = rr / pq (+ the pack launch the folded schedule left waiting)
    apply_bc(c, op->bc);
    StencilCall s2;
    LQCHK(make_full_call(op, po, w.tmp, 1, s2));          // update mode writes r only: `out` is a placeholder (the buffer that is dead until the p update)
    s2.gauge12t = gt;
    s2.gauge8t = w.links_t8;
    s2.sweep_rev = w.sweep_alt ? 1 : 0;      // (see cg_enqueue_rring)
    s2.keep_slabs = w.store_keep;
    s2.norm_partial = c->d_partial;
    if (fold) s2.scal_w = c->d_scal;
    s2.upd_scal = c->d_scal;
    s2.upd[0] = spinor_block(w.r, 0);
    s2.upd[1] = spinor_block(w.r, 1);
    if (fr) s2.red_slot = S_RRNEW;
    if (fp) s2.prepacked = 1;
    LQCHK(stencil_apply(c, s2));
    LQCHK(fr ? reduce_tail(c, 1, S_RRNEW, fold ? 0 : 2) : reduce_to_slot(c, nbs, 1, S_RRNEW, true, fold ? 0 : 2));   // + beta, convergence flag
    const int nbu = stream_grid(c, n);
    HArgs h = HArgs();
    int npx = 0, npack = 0;
    if (fp) {
        int nt = 0;
        for (int mu = 0; mu < 4; mu++)
            if (c->geom.part[mu]) nt = std::max(nt, 2 * face_half_sites(c->geom, mu));
        npx = (nt + UB - 1) / UB; npack = 8 * npx;
        h.g = c->geom;
        h.gauge = op->gauge->data;
        h.parity_mode = 2; h.dagger = 0;
        for (int q = 0; q < 2; q++) { h.in[q] = spinor_block(pk, q); h.upd[q] = spinor_block(w.r, q); }
        for (int mu = 0; mu < 4; mu++) {
            const size_t cnt = (size_t)2 * 6 * face_half_sites(c->geom, mu);      // [send_fwd | send_bwd] back to back (stencil.hip make_hargs)
            h.send_fwd[mu] = halo_send_base(c, mu, 0); h.send_bwd[mu] = halo_send_base(c, mu, 1) + cnt;
        }
    }
    const CgUpd u = {dim3(nbu + npack), x->data, pk->data, po->data, n, nbu, h, npx};
    if (!defer) hipLaunchKernelGGL(cg_update_xp, u.grid, dim3(UB), 0, c->stream, c->d_scal, x->data, w.p->data, w.r->data, n);
    else switch ((c->tun.nt_blas ? 4 : 0) | (fold ? 2 : 0) | (fp ? 1 : 0)) {
        case 0: cg_launch_update_defer<false, false, false>(c, w, u); break;
        case 1: cg_launch_update_defer<false, false, true>(c, w, u); break;
        case 2: cg_launch_update_defer<false, true, false>(c, w, u); break;
        case 3: cg_launch_update_defer<false, true, true>(c, w, u); break;
        case 4: cg_launch_update_defer<true, false, false>(c, w, u); break;
        case 5: cg_launch_update_defer<true, false, true>(c, w, u); break;
        case 6: cg_launch_update_defer<true, true, false>(c, w, u); break;
        default: cg_launch_update_defer<true, true, true>(c, w, u); break;
    }
    w.p_packed = fp;
    if (fp) w.pack_epoch = ++c->halo_epoch;
    HIPCHK(hipGetLastError());
    w.k++;
    return LQCD_OK;
}

int cg_enqueue_iteration(lqcd_op_s* op, lqcd_spinor_s* x, CgWork& w) {
    switch (w.form) {
        case CgForm::Reference: case CgForm::NormFused: return cg_iter_reference(op, x, w);
        case CgForm::Fused: case CgForm::DeferX: return cg_iter_fused(op, x, w);
        case CgForm::Small: return cg_iter_small(op, x, w);
        case CgForm::RRing: return cg_enqueue_rring(op, x, w);
        case CgForm::Unset: break;
    }
    set_error("CG: the work vectors were never set up (cg_setup fixes the iteration form)");
    return LQCD_ERR_ARG;
}

// the ring depth multiplier for this solve: the tunable cg_rring_mult, as long as K M <= RRING_MAX (the largest admissible M below it otherwise).  A context that never set
// the tunable keeps M = 1 in the launch-bound regime (<= 1024 stencil workgroups, where cg_small would apply): the deep ring was measured on lattices beyond it only.
static int cg_rring_mult_wanted(lqcd_op_s* op, int K) {
    lqcd_ctx_s* c = op->ctx;
    int M = c->tun.cg_rring_mult;
    if (!c->tun.cg_rring_mult_set && stencil_num_partials(c, op->kind, op->r, 2, 0, op_fused_clover(op)) <= 1024) M = 1;
    while (M > 1 && K * M > RRING_MAX) M >>= 1;
    return M;
}
// K - 2 more work vectors for a ring of K buffers (those already held are kept); K < 2 or a pool that cannot grow: none stay held, false
static bool cg_more_get(lqcd_ctx_s* c, CgWork& w, int K) {
    bool ok = K >= 2;
    for (int j = 0; j < K - 2 && ok; j++) {
        if (!w.more[j]) w.more[j] = scratch_get(c, w.r->kind, LQCD_FULL);
        ok = w.more[j] != nullptr;
    }
    if (!ok) for (lqcd_spinor_s*& f : w.more) { if (f) scratch_put(f); f = nullptr; }
    return ok;
}
// The one place the tunables pick the iteration form.  The small-lattice form first; then cg_fused = 3, the residual ring (its depth K M does not depend on `graph`: cg_run
// makes a captured burst a multiple of it) with its K M - 2 extra vectors -- M is halved while the pool cannot supply them, then the forms below; then the deferred x
// update; then by cg_fused.
static CgForm cg_choose_form(lqcd_op_s* op, CgWork& w) {
    lqcd_ctx_s* c = op->ctx;
    const int fused = c->tun.cg_fused;
    if (fused >= 2 && c->tun.cg_small && cg_small_ok(op, stencil_num_partials(c, op->kind, op->r, 2, 0, op_fused_clover(op)))) return CgForm::Small;
    if (const int K = cg_rring_wanted(op, w)) {
        for (int M = cg_rring_mult_wanted(op, K); M >= 1; M >>= 1)
            if (cg_more_get(c, w, K * M)) { w.rring = K * M; w.rring_k = K; return CgForm::RRing; }
    }
    if (fused >= 2 && c->tun.cg_defer_x) return CgForm::DeferX;
    return fused >= 2 ? CgForm::Fused : fused ? CgForm::NormFused : CgForm::Reference;
}

// The temporal-gauge solve reads 8 reals per link (lqcd_gauge_s::data8t) when EVERY stencil launch of it takes the TG8 instance -- the set-up applications, the plain D behind
// a batch, recurrence D and D^+: the residual-ring, Fused and DeferX forms -- the tunable cg_tgauge_recon says 8 (unset: beyond 1024 stencil workgroups only, so that small
// lattices keep the bits of the 12-real solve), and the 8-real copy of this version of the links exists and passed its gate (tgauge8_gate_e).  Anything else -- cg_small,
// the forms on op_apply_async, a failed gate or allocation -- reads 12 reals throughout: a solve never mixes the two operators.  Returns the copy, or nullptr.
static const double2* cg_tgauge8_links(lqcd_op_s* op, const CgWork& w) {
    lqcd_ctx_s* c = op->ctx;
    if (!w.tgauge || c->tun.cg_tgauge_recon != 8) return nullptr;
    if (!(w.form == CgForm::RRing || w.form == CgForm::Fused || w.form == CgForm::DeferX)) return nullptr;
    if (!c->tun.cg_tgauge_recon_set && stencil_num_partials(c, op->kind, op->r, 2, 0, op_fused_clover(op)) <= 1024) return nullptr;
    lqcd_gauge_s* g = op->gauge;
    if (gauge_ensure_tgauge(g, true) != LQCD_OK || !g->data8t) return nullptr;
    return g->tgauge8_dev <= std::pow(10.0, -(double)c->tun.tgauge8_gate_e) ? g->data8t : nullptr;
}

// bytes per site a stencil launch of the iteration moves in update or recurrence mode in temporal gauge: 288 of links (three directions of 12 reals), 192 each of neighbours, update source and store
// (192 of links in the 8-real solve: the store policy keeps its slab count in MB of the 12-real launch)
constexpr int CG_STENCIL_BYTES = 864;
int cg_setup(lqcd_op_s* op, lqcd_spinor_s* x, lqcd_spinor_s* b, CgWork& w, double eps, double* rr0) {
    lqcd_ctx_s* c = op->ctx;
    const size_t n = x->elems;
    LQCHK(halo_schedule_settle(op));      // the iteration counts |.|^2 partials: the halo schedule (folded or not) is fixed from here on
    // temporal gauge: x <- G x in place (cg_finish rotates it back), r = G b - D'^+ D' x without a write to b (it belongs to the caller)
    w.tgauge = cg_tgauge_wanted(op);
    c->tun.tgauge_active = w.tgauge ? 1 : 0;
    w.links_t = w.tgauge ? op->gauge->data12t : nullptr;
    w.gfix = w.tgauge ? op->gauge->gfix : nullptr;
    w.gauge_version = op->gauge->version;
    // the iteration form, ahead of the set-up applications: the link format of the whole solve hangs on it (RRing: sets the depth w.rring = K M and w.rring_k = K)
    w.rring = w.rring_k = 0;
    w.form = cg_choose_form(op, w);
    w.links_t8 = cg_tgauge8_links(op, w);
    c->tun.tgauge_recon_active = w.tgauge ? (w.links_t8 ? 8 : 12) : 0;
    if (w.tgauge) LQCHK(spinor_gauge_rotate(c, w.gfix, x->data, x->data, 0));
    // r = b - D^+ D x ; p = r
    LQCHK(op_apply_async(op, w.tmp, x, 0, nullptr, nullptr, w.links_t, w.links_t8));
    LQCHK(op_apply_async(op, w.q, w.tmp, 1, nullptr, nullptr, w.links_t, w.links_t8));
    if (w.tgauge) LQCHK(spinor_gauge_rotate(c, w.gfix, w.r->data, b->data, 0));
    else HIPCHK(hipMemcpyAsync(w.r->data, b->data, n * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
    LQCHK(blas_axpy(c, -1.0, 0.0, w.q->data, w.r->data, n));
    HIPCHK(hipMemcpyAsync(w.p->data, w.r->data, n * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
    LQCHK(blas_norm2(c, w.r->data, n, rr0, true));
    double init[12] = {*rr0, 0, 0, 0, 0, 0, eps, 0, 0, 0, 0, 0};   // S_RR .. S_XDONE, S_RROLD, S_APREV, S_BSTART
    static_assert(S_BSTART - S_RR == 11, "cg_setup: the scalar block it initialises ends at S_BSTART");
    HIPCHK(hipMemcpyAsync(c->d_scal + S_RR, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    w.k = 0; w.p_packed = false; w.flushed = false;
    c->tun.cg_rring_active = w.rring_k;
    c->tun.cg_rring_depth_active = w.rring;
    // the alternating sweep: the forms whose D^+ is a launch of the temporal-gauge instance (away from the seam it loads no time-like link, so no streaming hint sits on the
    // first use of one when t runs backwards).  Fixed here like the form: no iteration reads the tunable.
    w.sweep_alt = c->tun.cg_sweep_alt != 0 && w.tgauge && (w.form == CgForm::RRing || w.form == CgForm::Fused || w.form == CgForm::DeferX);
    c->tun.cg_sweep_alt_active = w.sweep_alt ? 1 : 0;
    // the store policy by slab rides on it: cg_store_keep_mb of launch traffic in slabs -- a slab is 1 / nslab of the lattice, and a stencil launch of the iteration moves
    // CG_STENCIL_BYTES per site (the 14 MB per slab of DESIGN section 4 at 32^3 x 64) -- clamped to [0, nslab].  Fixed here: a captured burst replays it unchanged
    w.store_keep = -1;
    if (w.sweep_alt && c->tun.cg_store_keep_mb >= 0 &&
        (c->tun.cg_store_keep_mb_set || stencil_num_partials(c, op->kind, op->r, 2, 0, op_fused_clover(op)) > 1024)) {
        const int nslab = stencil_sweep_slabs(c);
        if (nslab > 0) {
            const size_t slab_bytes = (size_t)CG_STENCIL_BYTES * (2 * (size_t)c->geom.Vh / nslab);
            w.store_keep = (int)std::min<size_t>(((size_t)c->tun.cg_store_keep_mb << 20) / slab_bytes, (size_t)nslab);
        }
    }
    c->tun.cg_store_keep_active = w.store_keep;
    w.ring = 2;
    if (w.form == CgForm::DeferX) {      // the ring of search-direction buffers (cg_defer_x = K): K - 2 more vectors, or the two-buffer form if the pool cannot grow
        int want = cg_ring_wanted(op);
        // a captured burst (tunable graph) replays the launches of iterations k = 0..7 with their buffer roles baked in: the ring must return to its starting state after
        // 8 iterations, i.e. divide the burst (K = 3, 5, 6, 7 silently broke the replay) -- otherwise the two-buffer form
        if (c->tun.graph != 0 && !any_partitioned(c) && (8 % want) != 0) want = 2;
        if (cg_more_get(c, w, want)) w.ring = want;
    }
    return LQCD_OK;
}

int cg_run(lqcd_op_s* op, lqcd_spinor_s* x, lqcd_spinor_s* b, double eps, int maxiter, bool fixed, int* iters, double* final_rr) {
    lqcd_ctx_s* c = op->ctx;
    HIPCHK(hipSetDevice(c->device));
    CgWork w;
    int st = cg_work_get(c, x->kind, w);
    double rr = 0;
    int it = 0;
    bool converged = false;
    // launch-bound staggered lattices: initial residual and all iterations in one launch (cg_persist.hip); x is complete on return
    bool one_launch = st == LQCD_OK && maxiter > 0 && c->tun.graph == 0 && cg_persist_ok(op);
    if (one_launch) {
        bool gave_up = false;
        st = cg_persist_run(op, x, b, w, fixed ? -1.0 : eps, maxiter, &it, &rr, &converged, &gave_up);
        if (gave_up) { one_launch = false; it = 0; rr = 0; converged = false; c->tun.cg_persist = 0; }      // not all workgroups were resident: the chain from here on
        else if (st == LQCD_OK && !std::isfinite(rr)) { set_error("CG: residual is not finite"); st = LQCD_ERR_NOT_CONVERGED; }
    }
    if (st == LQCD_OK && !one_launch) st = cg_setup(op, x, b, w, fixed ? -1.0 : eps, &rr);
    if (st == LQCD_OK && !one_launch && !fixed && rr < eps) converged = true;
    int check_every = 8;
    // Launch-bound lattices (the cg_small regime: <= 1024 stencil workgroups, an iteration is three ~5 us launches): every readback of the
    // scalar block is a host synchronisation worth about two iterations, an iteration enqueued behind the converging one only three no-op
    // launches.  There the burst length follows the observed convergence rate -- enough iterations to reach eps by the rate of the last
    // burst, at most 32 -- instead of a fixed 8.  The returned iterate and count do not depend on the burst length (done-flag protocol).
    const bool adaptive = !fixed && c->tun.graph == 0 && w.form == CgForm::Small;
    int next_burst = check_every, it_prev = 0;
    double rr_prev = rr;
    // tunable "graph": a burst of check_every iterations is captured once into a hipGraph and replayed -- one launch per
    // burst instead of 5 per iteration.  Pays on launch-bound (small) lattices; single-stream (unpartitioned) contexts only.
    const bool use_graph = c->tun.graph != 0 && !any_partitioned(c) && !(c->has_comm && c->peer.on);      // (the peer-mapped reductions carry a sequence number per launch)
    // residual ring: a replayed burst bakes the slot roles in, so it must leave the ring where it found it -- the captured burst is the multiple of the depth K M at or
    // above 8 (8 for K M = 2, 4, 8; 16; 32).  The surplus iterations behind the converging one are no-ops (done flag): iterate and count do not depend on the burst length.
    if (use_graph && w.form == CgForm::RRing && w.rring > 0) check_every = (check_every + w.rring - 1) / w.rring * w.rring;
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    while (st == LQCD_OK && !one_launch && !converged && it < maxiter) {
        int burst = std::min(adaptive ? next_burst : check_every, maxiter - it);
        if (fixed && !use_graph) burst = maxiter - it;
        if (use_graph && burst == check_every) {
            if (!gexec) {
                if (c->tun.halo_stream_mode < 0) c->tun.halo_stream_mode = 0;    // the auto-tuning pass synchronises: not inside a capture
                hipError_t ge = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
                if (ge != hipSuccess) { st = hip_fail(ge, "hipStreamBeginCapture", __FILE__, __LINE__); break; }
                for (int k = 0; k < burst && st == LQCD_OK; k++) st = cg_enqueue_iteration(op, x, w);
                ge = hipStreamEndCapture(c->stream, &graph);
                if (st == LQCD_OK && ge != hipSuccess) st = hip_fail(ge, "hipStreamEndCapture", __FILE__, __LINE__);
                if (st == LQCD_OK) {
                    ge = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
                    if (ge != hipSuccess) st = hip_fail(ge, "hipGraphInstantiate", __FILE__, __LINE__);
                }
                if (st != LQCD_OK) break;
            }
            hipError_t ge = hipGraphLaunch(gexec, c->stream);
            if (ge != hipSuccess) { st = hip_fail(ge, "hipGraphLaunch", __FILE__, __LINE__); break; }
        } else {
            for (int k = 0; k < burst && st == LQCD_OK; k++) st = cg_enqueue_iteration(op, x, w);
        }
        if (st != LQCD_OK) break;
        if (fixed && use_graph && it + burst < maxiter) { it += burst; continue; }   // timing window: no readback between bursts
        hipError_t e = hipMemcpyAsync(c->h_scal, c->d_scal + S_RR, 8 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { st = hip_fail(e, "cg scalar readback", __FILE__, __LINE__); break; }
        rr = c->h_scal[S_RR - S_RR];
        it = (int)c->h_scal[S_ITERS - S_RR];
        if (c->h_scal[S_DONE - S_RR] != 0.0) converged = true;
        if (!std::isfinite(rr)) { set_error("CG: residual is not finite"); st = LQCD_ERR_NOT_CONVERGED; }
        if (adaptive && !converged && it > it_prev && rr > 0.0 && rr < rr_prev) {
            const double per_it = std::log(rr / rr_prev) / (double)(it - it_prev);     // < 0
            const double need = std::log(eps / rr) / per_it;
            next_burst = (int)std::min(32.0, std::max(2.0, std::ceil(need)));
        } else if (adaptive) {
            next_burst = check_every;
        }
        it_prev = it; rr_prev = rr;
    }
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (graph) (void)hipGraphDestroy(graph);
    if (!one_launch && (w.tgauge || (st == LQCD_OK && (!converged || w.form == CgForm::RRing)))) {      // a window / an exhausted solve that stopped on an even iteration: complete x (residual ring: also behind the converging iteration); temporal gauge: x back to the caller's basis
        const int fs = cg_finish(op, x, w, st == LQCD_OK && (!converged || w.form == CgForm::RRing));
        if (st == LQCD_OK) st = fs;
        if (st == LQCD_OK) { hipError_t e = hipStreamSynchronize(c->stream); if (e != hipSuccess) st = hip_fail(e, "cg flush", __FILE__, __LINE__); }
    }
    cg_work_put(w);
    if (iters) *iters = it;
    if (final_rr) *final_rr = rr;
    if (st != LQCD_OK) { c->has_waiting_pack = false; return st; }      // (a pack left waiting by the failed iteration names work vectors that went back to the pool)
    if (comm_check(c) != LQCD_OK) return LQCD_ERR_COMM;                 // peer-mapped backend: a wait gave up (dead rank)
    if (!fixed && !converged) {
        set_error("The CG is not converged! maxsteps = " + std::to_string(maxiter) + ", residual = " + std::to_string(rr));
        return LQCD_ERR_NOT_CONVERGED;
    }
    return LQCD_OK;
}

}  // namespace lqcd

using namespace lqcd;

// ---------------------------------------------------------------------------------- C API: solvers
extern "C" int lqcd_solve_cg_DdagD(lqcd_op_t op, lqcd_spinor_t x, lqcd_spinor_t b, double eps, int maxiter, int* iters, double* final_rr) {
    if (op && op->kind == LQCD_DOMAINWALL) return dw_solve_cg(op, x, b, eps, maxiter, iters, final_rr);
    LQCHK(check_full(op, x, b, "lqcd_solve_cg_DdagD"));
    ARGCHK(maxiter >= 0, "lqcd_solve_cg_DdagD: maxiter < 0");
    return cg_run(op, x, b, eps, maxiter, false, iters, final_rr);
}
extern "C" int lqcd_solve_cg_DdagD_fixed(lqcd_op_t op, lqcd_spinor_t x, lqcd_spinor_t b, int niter) {
    LQCHK(check_full(op, x, b, "lqcd_solve_cg_DdagD_fixed"));
    return cg_run(op, x, b, 0.0, niter, true, nullptr, nullptr);
}


// CG with device-resident scalars for a Hermitian positive operator given as an enqueue function (reference form:
// alpha = rr / <p, A p>); x holds the initial guess, work = three fields of n elements.  Used where the fused full-lattice
// iteration of cg_run does not apply (parity blocks).
int lqcd::cg_launch_update_xp(lqcd_ctx_s* c, double2* x, double2* p, const double2* r, size_t n) {
    hipLaunchKernelGGL(cg_update_xp, dim3(stream_grid(c, n)), dim3(UB), 0, c->stream, c->d_scal, x, p, r, n);
    HIPCHK(hipGetLastError());
    return LQCD_OK;
}

int lqcd::cg_generic(lqcd_ctx_s* c, const ApplyFn& A, size_t n, double2* x, const double2* b, double2* r, double2* p, double2* q, double eps,
                     int maxiter, int* iters, double* final_rr) {
    LQCHK(A(q, x));
    HIPCHK(hipMemcpyAsync(r, b, n * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
    LQCHK(blas_axpy(c, -1.0, 0.0, q, r, n));
    HIPCHK(hipMemcpyAsync(p, r, n * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
    double rr = 0;
    LQCHK(blas_norm2(c, r, n, &rr, true));
    double init[9] = {rr, 0, 0, 0, 0, 0, eps, 0, 0};   // S_RR .. S_XDONE
    HIPCHK(hipMemcpyAsync(c->d_scal + S_RR, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int it = 0;
    bool converged = rr < eps;
    const int check_every = 8;
    while (!converged && it < maxiter) {
        const int burst = std::min(check_every, maxiter - it);
        for (int k = 0; k < burst; k++) {
            LQCHK(A(q, p));
            LQCHK(cg_plain_tail(c, x, r, p, q, n, true));
        }
        HIPCHK(hipMemcpyAsync(c->h_scal, c->d_scal + S_RR, 8 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        rr = c->h_scal[0];
        it = (int)c->h_scal[S_ITERS - S_RR];
        if (c->h_scal[S_DONE - S_RR] != 0.0) converged = true;
        if (!std::isfinite(rr)) { set_error("CG: residual is not finite"); return LQCD_ERR_NOT_CONVERGED; }
    }
    if (iters) *iters = it;
    if (final_rr) *final_rr = rr;
    if (!converged) {
        set_error("The CG is not converged! maxsteps = " + std::to_string(maxiter) + ", residual = " + std::to_string(rr));
        return LQCD_ERR_NOT_CONVERGED;
    }
    return LQCD_OK;
}

// Staggered D^+D = m^2 - H^2 is block diagonal in parity: (D^+D)_pp = m^2 - H_pq H_qp.  Solves that block for the parity-p halves of
// the FULL fields x (initial guess / solution) and b with half-lattice vectors -- one Dslash-equivalent per iteration instead of
// two.  The other parity of x is not touched.  This is the solve behind the reference's "4 tastes" (Nf = 4) staggered action, whose
// pseudofermion lives on the even sites (test/test_staggered.toml).
extern "C" int lqcd_solve_cg_DdagD_parity(lqcd_op_t op, lqcd_spinor_t x, lqcd_spinor_t b, int parity, double eps, int maxiter, int* iters,
                                          double* final_rr) {
    LQCHK(check_full(op, x, b, "lqcd_solve_cg_DdagD_parity"));
    ARGCHK(op->kind == LQCD_STAGGERED && (parity == 0 || parity == 1) && maxiter >= 0,
           "lqcd_solve_cg_DdagD_parity: staggered operators only, parity 0 (even) or 1 (odd)");
    lqcd_ctx_s* c = op->ctx;
    HIPCHK(hipSetDevice(c->device));
    apply_bc(c, op->bc);
    const size_t nh = x->elems / 2;
    const int mine = parity ? LQCD_ODD : LQCD_EVEN, other = parity ? LQCD_EVEN : LQCD_ODD;
    ScratchScope pool(c);
    lqcd_spinor_s *r = pool.get(op->kind, mine), *p = pool.get(op->kind, mine), *q = pool.get(op->kind, mine), *t = pool.get(op->kind, other);
    if (!(r && p && q && t)) return LQCD_ERR_HIP;
    lqcd_spinor_s xv = *x, bv = *b;
    xv.subset = bv.subset = mine;
    xv.elems = bv.elems = nh;
    xv.data = x->data + (size_t)parity * nh;
    bv.data = b->data + (size_t)parity * nh;
    lqcd_spinor_s vin = xv, vout = xv;
    const double m2 = op->km * op->km;
    ApplyFn A = [&](double2* out, const double2* in) -> int {
        vin.data = const_cast<double2*>(in);
        vout.data = out;
        StencilCall s1 = make_hop_call(op, t, &vin, nullptr, 0.0, 1.0, 0);          // t = H in (other parity)
        LQCHK(stencil_apply(c, s1));
        StencilCall s2 = make_hop_call(op, &vout, t, &vin, m2, -1.0, 0);            // out = m^2 in - H t
        return stencil_apply(c, s2);
    };
    return cg_generic(c, A, nh, xv.data, bv.data, r->data, p->data, q->data, eps, maxiter, iters, final_rr);
}
