// bicgstab_eo.hip -- even-odd (Schur) preconditioned BiCGStab of the Wilson / Wilson-clover operator: the fused chain (tunable bicg_fused) and its entry point.
//
// Replaces, behind the C ABI, LatticeDiracOperators.jl's even-odd solve_DinvX! -- SURVEY.md 8(a) a5.
#include "ops_internal.h"

#include <algorithm>
#include <cmath>

namespace lqcd {

// ---------------------------------------------------------------------------------- even-odd BiCGStab, plain Wilson: the fused chain (tunable bicg_fused)
// The Schur operator M = 1 - k^2 H_eo H_oe is two hops; its SECOND hop forms the inner product an iteration needs next in its epilogue
// (StencilCall::dot_z: <r0, v> with v = M p, and <t, s>, |t|^2 with t = M s), so no pass over the vectors exists only to multiply them.
// fold (lattices of <= 1024 chunks per parity, where an iteration is a chain of short dependent launches): the block partials of a producer are
// summed by EVERY workgroup of the consumer in its prologue (sum_partials_small_nv: the order of the one-block reduction kernel) and the scalar
// steps (bicg_alpha / bicg_omega / bicg_beta, shared with the scalar kernels of blas.hip) run there too:
//     hop, hop+<r0,v> | s = r - alpha v, |s|^2 | hop, hop+<t,s>,|t|^2 | x += alpha p + omega s, r = s - omega t, |r|^2, <r0,r> | p = r + beta (p - omega v)
// = 7 dependent launches per iteration instead of 17, the same bits in every vector as the unfolded form (partials, summation order and scalar
// expressions are the same; tests/test_gpu_solver_edges.py).  rho lives in two slots used alternately: block 0 of the p update writes the new value
// while the other workgroups still read the old one.
// The three streaming kernels request the first KE elements of every thread BEFORE the prologue (whose partial sums are a memory round trip of their
// own and do not depend on them), then walk the rest of a large vector in the usual grid-stride loop: same element -> thread map, same order of the
// per-thread additions, hence the same partials whether the prologue folds a reduction or not.
constexpr int KE = 3;
// s = r - alpha v ; partial |s|^2          (fold: alpha = rho / <r0, v> from the partials of the Schur operator's epilogue)
__global__ __launch_bounds__(UB) void bicgf_s(BicgF a, double2* __restrict__ s, const double2* __restrict__ r, const double2* __restrict__ v, size_t n) {
    if (a.sc[B_DONE] != 0.0) { if (blockIdx.x == 0 && threadIdx.x == 0) a.sc[B_XDONE] = 1.0; return; }      // raised by an EARLIER launch: its update is complete (B_XDONE, lqcd_internal.h)
    const size_t i0 = (size_t)blockIdx.x * UB + threadIdx.x, stride = (size_t)gridDim.x * UB;
    double2 pr[KE], pv[KE];
#pragma unroll
    for (int e = 0; e < KE; e++) {
        const size_t i = i0 + e * stride;
        if (i < n) { pr[e] = r[i]; pv[e] = v[i]; }
    }
    // the sums: from the producer's partials (fold) or from the slots a one-block reduction launch filled; the scalar step is formed HERE in both
    // forms -- the same instructions, hence the same bits
    c2 r0v, rho = {a.sc[a.rho_in], a.sc[a.rho_in + 1]};
    if (a.fold) {
        double t3[3];
        block_sum_partials<3>(a.pin, a.pin_n, t3, a.pin_soa != 0);
        r0v.re = t3[0]; r0v.im = t3[1];
    } else { r0v.re = a.sc[B_R0V]; r0v.im = a.sc[B_R0V + 1]; }
    const c2 al = bicg_alpha(rho, r0v);
    if (a.pin3 && a.sc[B_UNSURE] != 0.0) {      // bicg_fused = 4: the last update launch left the stopping test to the |r'|^2 it summed (every workgroup reaches the same verdict)
        double t1[1];
        block_sum_partials<1>(a.pin3, a.pin3_n, t1);
        if (blockIdx.x == 0 && threadIdx.x == 0) { a.sc[B_RES] = t1[0]; a.sc[B_RR] = t1[0]; }
        if (t1[0] < a.sc[B_EPS]) { if (blockIdx.x == 0 && threadIdx.x == 0) { a.sc[B_DONE] = 1.0; a.sc[B_XDONE] = 1.0; } return; }      // (the update it judges was the last launch's)
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.sc[B_R0V] = r0v.re; a.sc[B_R0V + 1] = r0v.im; a.sc[B_ALPHA] = al.re; a.sc[B_ALPHA + 1] = al.im; }
    const double ar = al.re, ai = al.im;
    double acc[1] = {0};
    auto one = [&](size_t i, double2 sv, const double2 vv) {
        sv.x = fma(-ar, vv.x, sv.x); sv.x = fma(ai, vv.y, sv.x);
        sv.y = fma(-ar, vv.y, sv.y); sv.y = fma(-ai, vv.x, sv.y);
        s[i] = sv;
        acc[0] = fma(sv.x, sv.x, acc[0]); acc[0] = fma(sv.y, sv.y, acc[0]);
    };
#pragma unroll
    for (int e = 0; e < KE; e++) {
        const size_t i = i0 + e * stride;
        if (i < n) one(i, pr[e], pv[e]);
    }
    for (size_t i = i0 + KE * stride; i < n; i += stride) one(i, r[i], v[i]);
    block_reduce_nv<1>(acc, a.pout);
}
// x += alpha p + omega s ; r = s - omega t ; partials |r|^2, <r0, r>       (fold: half-step test on |s|^2 and omega = <t, s> / |t|^2 in the prologue)
__global__ __launch_bounds__(UB) void bicgf_xr(BicgF a, double2* __restrict__ x, double2* __restrict__ r, const double2* __restrict__ p,
                                                const double2* __restrict__ s, const double2* __restrict__ t, const double2* __restrict__ r0, size_t n) {
    if (a.sc[B_DONE] != 0.0) return;
    const size_t i0 = (size_t)blockIdx.x * UB + threadIdx.x, stride = (size_t)gridDim.x * UB;
    double2 pp[KE], ps[KE], pt[KE], pz[KE], px[KE];
#pragma unroll
    for (int e = 0; e < KE; e++) {
        const size_t i = i0 + e * stride;
        if (i < n) { pp[e] = p[i]; ps[e] = s[i]; pt[e] = t[i]; pz[e] = r0[i]; px[e] = x[i]; }
    }
    const double ar = a.sc[B_ALPHA], ai = a.sc[B_ALPHA + 1];
    double ss, tt;
    c2 ts;
    if (a.fold) {
        double t1[1], t3[3];
        block_sum_partials<1>(a.pin2, a.pin2_n, t1);
        block_sum_partials<3>(a.pin, a.pin_n, t3, a.pin_soa != 0);
        ss = t1[0]; ts.re = t3[0]; ts.im = t3[1]; tt = t3[2];
    } else { ss = a.sc[B_SS]; ts.re = a.sc[B_TS]; ts.im = a.sc[B_TS + 1]; tt = a.sc[B_TT]; }
    const bool half = ss < a.sc[B_EPS];
    const c2 om = bicg_omega(ts, tt, half);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.sc[B_SS] = ss; a.sc[B_HALF] = half ? 1.0 : 0.0; a.sc[B_TS] = ts.re; a.sc[B_TS + 1] = ts.im; a.sc[B_TT] = tt;
        a.sc[B_OMEGA] = om.re; a.sc[B_OMEGA + 1] = om.im;
    }
    const double wr = om.re, wi = om.im;
    double acc[3] = {0, 0, 0};
    auto one = [&](size_t i, const double2 pv, const double2 sv, const double2 tv, const double2 zv, double2 xv) {
        double2 rv = sv;
        xv.x = fma(ar, pv.x, xv.x); xv.x = fma(-ai, pv.y, xv.x);
        xv.y = fma(ar, pv.y, xv.y); xv.y = fma(ai, pv.x, xv.y);
        xv.x = fma(wr, sv.x, xv.x); xv.x = fma(-wi, sv.y, xv.x);
        xv.y = fma(wr, sv.y, xv.y); xv.y = fma(wi, sv.x, xv.y);
        rv.x = fma(-wr, tv.x, rv.x); rv.x = fma(wi, tv.y, rv.x);
        rv.y = fma(-wr, tv.y, rv.y); rv.y = fma(-wi, tv.x, rv.y);
        x[i] = xv; r[i] = rv;
        acc[0] = fma(rv.x, rv.x, acc[0]); acc[0] = fma(rv.y, rv.y, acc[0]);
        acc[1] = fma(zv.x, rv.x, acc[1]); acc[1] = fma(zv.y, rv.y, acc[1]);
        acc[2] = fma(zv.x, rv.y, acc[2]); acc[2] = fma(-zv.y, rv.x, acc[2]);
    };
#pragma unroll
    for (int e = 0; e < KE; e++) {
        const size_t i = i0 + e * stride;
        if (i < n) one(i, pp[e], ps[e], pt[e], pz[e], px[e]);
    }
    for (size_t i = i0 + KE * stride; i < n; i += stride) one(i, p[i], s[i], t[i], r0[i], x[i]);
    block_reduce_nv<3>(acc, a.pout);
}
// p = r + beta (p - omega v)       (fold: iteration count, convergence / breakdown and beta = (rho'/rho)(alpha/omega) in the prologue)
__global__ __launch_bounds__(UB) void bicgf_p(BicgF a, double2* __restrict__ p, const double2* __restrict__ r, const double2* __restrict__ v, size_t n) {
    if (a.sc[B_DONE] != 0.0) return;
    const size_t i0 = (size_t)blockIdx.x * UB + threadIdx.x, stride = (size_t)gridDim.x * UB;
    double2 pv_[KE], pr[KE], pp[KE];
#pragma unroll
    for (int e = 0; e < KE; e++) {
        const size_t i = i0 + e * stride;
        if (i < n) { pv_[e] = v[i]; pr[e] = r[i]; pp[e] = p[i]; }
    }
    const double wr = a.sc[B_OMEGA], wi = a.sc[B_OMEGA + 1];
    const bool half = a.sc[B_HALF] != 0.0;
    double rrn;
    c2 rho1, rho = {a.sc[a.rho_in], a.sc[a.rho_in + 1]}, al = {a.sc[B_ALPHA], a.sc[B_ALPHA + 1]}, om = {wr, wi};
    if (a.fold) {
        double t3[3];
        block_sum_partials<3>(a.pin, a.pin_n, t3);
        rrn = t3[0]; rho1.re = t3[1]; rho1.im = t3[2];
    } else { rrn = a.sc[B_RR]; rho1.re = a.sc[B_RHO1]; rho1.im = a.sc[B_RHO1 + 1]; }
    const double rr = half ? a.sc[B_SS] : rrn;
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    if (lead) { a.sc[B_ITERS] += 1.0; a.sc[B_RES] = rr; a.sc[B_RR] = rrn; a.sc[B_RHO1] = rho1.re; a.sc[B_RHO1 + 1] = rho1.im; }
    if (half || rr < a.sc[B_EPS]) { if (lead) a.sc[B_DONE] = 1.0; return; }
    if (!(fabs(rr) <= 1.79e308)) { if (lead) a.sc[B_DONE] = 2.0; return; }      // NaN / inf: breakdown
    const c2 be = bicg_beta(rho1, rho, al, om);
    if (lead) { a.sc[B_BETA] = be.re; a.sc[B_BETA + 1] = be.im; a.sc[a.rho_out] = rho1.re; a.sc[a.rho_out + 1] = rho1.im; }
    const double br = be.re, bi = be.im;
    auto one = [&](size_t i, const double2 vv, const double2 rv, double2 pv) {
        pv.x = fma(-wr, vv.x, pv.x); pv.x = fma(wi, vv.y, pv.x);
        pv.y = fma(-wr, vv.y, pv.y); pv.y = fma(-wi, vv.x, pv.y);
        double2 o;
        o.x = fma(br, pv.x, rv.x); o.x = fma(-bi, pv.y, o.x);
        o.y = fma(br, pv.y, rv.y); o.y = fma(bi, pv.x, o.y);
        p[i] = o;
    };
#pragma unroll
    for (int e = 0; e < KE; e++) {
        const size_t i = i0 + e * stride;
        if (i < n) one(i, pv_[e], pr[e], pp[e]);
    }
    for (size_t i = i0 + KE * stride; i < n; i += stride) one(i, v[i], r[i], p[i]);
}

// bicg_fused = 4: x / r update and p update as ONE launch WITHOUT a barrier.  What the p update needs from the new residual -- rho' = <r0, r'> and the stopping test --
// follows from inner products that exist before r' does:  r' = s - omega t and s = r - alpha v give
//     rho' = rho - alpha <r0, v> - omega <r0, t> ,        |r'|^2 = |s|^2 - |<t, s>|^2 / |t|^2
// with <r0, t> formed next to <t, s>, |t|^2 in the epilogue of the Schur operator's second hop (StencilCall::dot_z2: five values per workgroup).  One launch, one
// reduction and two vector passes less per iteration than bicg_fused = 2 (x, p, s, t, v read, x, r, p written; r0 is read by the hop instead of here).  The iterates
// equal those of the other forms up to the rounding of the two recurrences (fp64: ~1e-16 of |r0| |r| per iteration, tests/test_gpu_solver_edges.py); the
// stopping test trusts the recurrence for |r'|^2 only while it is free of cancellation (|r'|^2 > 1e-6 |s|^2), otherwise this launch also sums the |r'|^2 it
// writes and the NEXT iteration's first streaming kernel decides (bicgf_s, a.pin3; the two hops in between are wasted once).
// The done flag travels in two stages: the lead raises B_DONE here (hops, bicgf_s and the host look at it), bicgf_s of the next iteration promotes it to B_XDONE, and
// only B_XDONE turns this launch into a no-op -- a workgroup that starts after the lead's store still applies the last update.
__global__ __launch_bounds__(UB) void bicgf_xrp_rec(BicgF a, double2* __restrict__ x, double2* __restrict__ r, double2* __restrict__ p, const double2* __restrict__ s,
                                                     const double2* __restrict__ t, const double2* __restrict__ v, size_t n) {
    if (a.sc[B_XDONE] != 0.0) return;      // NOT B_DONE: the lead of this launch raises it below while other workgroups have not started, and they owe x the converging iteration's update
    const size_t i0 = (size_t)blockIdx.x * UB + threadIdx.x, stride = (size_t)gridDim.x * UB;
    double2 pp[KE], ps[KE], pt[KE], px[KE], pv_[KE];
#pragma unroll
    for (int e = 0; e < KE; e++) {
        const size_t i = i0 + e * stride;
        if (i < n) { pp[e] = p[i]; ps[e] = s[i]; pt[e] = t[i]; px[e] = x[i]; pv_[e] = v[i]; }
    }
    const c2 al = {a.sc[B_ALPHA], a.sc[B_ALPHA + 1]}, rho = {a.sc[a.rho_in], a.sc[a.rho_in + 1]}, r0v = {a.sc[B_R0V], a.sc[B_R0V + 1]};
    double ss, tt;
    c2 ts, r0t;
    if (a.fold == 1) {
        double t1[1], t5[5];
        block_sum_partials<1>(a.pin2, a.pin2_n, t1);
        block_sum_partials<5>(a.pin, a.pin_n, t5, a.pin_soa != 0);
        ss = t1[0]; ts.re = t5[0]; ts.im = t5[1]; tt = t5[2]; r0t.re = t5[3]; r0t.im = t5[4];
    } else {
        if (a.fold == 2) { double t1[1]; block_sum_partials<1>(a.pin2, a.pin2_n, t1); ss = t1[0]; }      // large lattices: the <= 1024 partials of |s|^2 are still summed here (one launch less)
        else ss = a.sc[B_SS];
        ts.re = a.sc[B_TS5]; ts.im = a.sc[B_TS5 + 1]; tt = a.sc[B_TS5 + 2]; r0t.re = a.sc[B_TS5 + 3]; r0t.im = a.sc[B_TS5 + 4];
    }
    const bool half = ss < a.sc[B_EPS];
    const c2 om = bicg_omega(ts, tt, half);
    // rho' = rho - alpha <r0, v> - omega <r0, t>
    c2 rho1;
    rho1.re = rho.re - (al.re * r0v.re - al.im * r0v.im) - (om.re * r0t.re - om.im * r0t.im);
    rho1.im = rho.im - (al.re * r0v.im + al.im * r0v.re) - (om.re * r0t.im + om.im * r0t.re);
    const double rrn = half ? ss : ss - (ts.re * ts.re + ts.im * ts.im) / tt;
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    const bool finite = fabs(rrn) <= 1.79e308 && fabs(ss) <= 1.79e308;
    const bool done = half || (finite && rrn < a.sc[B_EPS] && rrn > a.guard * ss);
    const bool unsure = !half && finite && !(rrn > a.guard * ss);      // the recurrence for |r'|^2 has cancelled six digits: the sum below decides, one kernel later
    if (lead) {
        a.sc[B_SS] = ss; a.sc[B_HALF] = half ? 1.0 : 0.0; a.sc[B_TS] = ts.re; a.sc[B_TS + 1] = ts.im; a.sc[B_TT] = tt;
        a.sc[B_OMEGA] = om.re; a.sc[B_OMEGA + 1] = om.im;
        a.sc[B_ITERS] += 1.0; a.sc[B_RES] = rrn; a.sc[B_RR] = rrn; a.sc[B_RHO1] = rho1.re; a.sc[B_RHO1 + 1] = rho1.im;
        if (done) a.sc[B_DONE] = 1.0;
        else if (!finite) a.sc[B_DONE] = 2.0;
    }
    const double ar = al.re, ai = al.im, wr = om.re, wi = om.im;
    c2 be = {0.0, 0.0};
    const bool go_on = !done && finite;
    if (go_on) {
        be = bicg_beta(rho1, rho, al, om);
        if (lead) { a.sc[B_BETA] = be.re; a.sc[B_BETA + 1] = be.im; a.sc[a.rho_out] = rho1.re; a.sc[a.rho_out + 1] = rho1.im; }
    }
    const double br = be.re, bi = be.im;
    double acc[1] = {0};
    auto one = [&](size_t i, double2 pv, const double2 sv, const double2 tv, double2 xv, const double2 vv) {
        double2 rv = sv;
        xv.x = fma(ar, pv.x, xv.x); xv.x = fma(-ai, pv.y, xv.x);
        xv.y = fma(ar, pv.y, xv.y); xv.y = fma(ai, pv.x, xv.y);
        xv.x = fma(wr, sv.x, xv.x); xv.x = fma(-wi, sv.y, xv.x);
        xv.y = fma(wr, sv.y, xv.y); xv.y = fma(wi, sv.x, xv.y);
        rv.x = fma(-wr, tv.x, rv.x); rv.x = fma(wi, tv.y, rv.x);
        rv.y = fma(-wr, tv.y, rv.y); rv.y = fma(-wi, tv.x, rv.y);
        x[i] = xv; r[i] = rv;
        acc[0] = fma(rv.x, rv.x, acc[0]); acc[0] = fma(rv.y, rv.y, acc[0]);
        if (go_on) {
            pv.x = fma(-wr, vv.x, pv.x); pv.x = fma(wi, vv.y, pv.x);
            pv.y = fma(-wr, vv.y, pv.y); pv.y = fma(-wi, vv.x, pv.y);
            double2 o;
            o.x = fma(br, pv.x, rv.x); o.x = fma(-bi, pv.y, o.x);
            o.y = fma(br, pv.y, rv.y); o.y = fma(bi, pv.x, o.y);
            p[i] = o;
        }
    };
#pragma unroll
    for (int e = 0; e < KE; e++) {
        const size_t i = i0 + e * stride;
        if (i < n) one(i, pp[e], ps[e], pt[e], px[e], pv_[e]);
    }
    for (size_t i = i0 + KE * stride; i < n; i += stride) one(i, p[i], s[i], t[i], x[i], v[i]);
    if (unsure) block_reduce_nv<1>(acc, a.pout);      // (uniform over the grid: every workgroup computed the same scalars)
    if (lead) a.sc[B_UNSURE] = unsure ? 1.0 : 0.0;    // "the sum of |r'|^2 in a.pout is waiting for a verdict"
}

// start of a solve in two launches and no host round trip (round 6; it used to be three copies, an axpy, a norm, a reduction, a read-back and an upload of the scalar
// block: 135 us in front of the first iteration of a 12-iteration solve at 16^3x32): r = rhs - v (v = M x0), r0 = r, p = r, |r|^2 partials ...
__global__ __launch_bounds__(UB) void bicgf_init(double2* __restrict__ r, double2* __restrict__ r0, double2* __restrict__ p, const double2* __restrict__ rhs,
                                                  const double2* __restrict__ v, size_t n, double* partial) {      // v == nullptr: zero guess, r = rhs
    double acc[1] = {0};
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        const double2 b = rhs[i], q = v ? v[i] : make_double2(0.0, 0.0);
        double2 o;
        o.x = b.x - q.x; o.y = b.y - q.y;
        r[i] = o; r0[i] = o; p[i] = o;
        acc[0] = fma(o.x, o.x, acc[0]); acc[0] = fma(o.y, o.y, acc[0]);
    }
    block_reduce_nv<1>(acc, partial);
}
// ... and the scalar block of the chain from their sum (<= 1024 partials, one wave): rho = rho' = |r|^2, eps, the residual, done if it is below eps already
__global__ __launch_bounds__(64) void bicgf_init_scal(const double* __restrict__ partial, int nb, double* sc, double eps) {
    const double rr = sum_partials_small_nv(partial, nb, 1, 0);
    if (threadIdx.x == 0) {
        for (int j = B_RHO; j < B_END; j++) sc[j] = 0.0;
        sc[B_RHO] = rr; sc[B_RHOB] = rr; sc[B_EPS] = eps; sc[B_RES] = rr;
        if (rr < eps) { sc[B_DONE] = 1.0; sc[B_XDONE] = 1.0; }
    }
}

// xe = M^-1 rhs on the even sites, M = 1 - k^2 H_eo H_oe (dagger: H -> H^+).  w[0..5] = r, r0, p, v, s, t; to: an odd-parity work vector.
// Same recurrences, stopping rule (|s|^2 < eps half-step exit, |r|^2 < eps) and iteration count as bicgstab_core.
// Ai != nullptr: Wilson-clover, M = 1 - k^2 A_ee^-1 H_eo A_oo^-1 H_oe with the packed inverse blocks applied to the hop sums inside the two hops
// (StencilCall::clover_on_hop) -- still two launches per M, no intermediate field.
int schur_wilson(lqcd_op_s* op, lqcd_spinor_s* out, lqcd_spinor_s* in, lqcd_spinor_s* to, int dg, const double2* Ai) {      // out = (1 - k^2 [A_ee^-1] H_eo [A_oo^-1] H_oe) in, fp64
    lqcd_ctx_s* c = op->ctx;
    StencilCall s1 = make_hop_call(op, to, in, nullptr, 0.0, 1.0, dg);
    if (Ai) { s1.clover = Ai; s1.clover_on_hop = 1; }
    LQCHK(stencil_apply(c, s1));
    StencilCall s2 = make_hop_call(op, out, to, in, 1.0, -op->km * op->km, dg);
    if (Ai) { s2.clover = Ai; s2.clover_on_hop = 1; }
    return stencil_apply(c, s2);
}
int bicgstab_eo_wilson(lqcd_op_s* op, lqcd_spinor_s& xe, lqcd_spinor_s* rhs, lqcd_spinor_s* const w[6], lqcd_spinor_s* to, int dg, double eps,
                       int maxiter, int* iters, double* final_rr, const double2* Ai) {
    lqcd_ctx_s* c = op->ctx;
    const double k = op->km;
    const size_t n = xe.elems, bytes = n * sizeof(double2);
    lqcd_spinor_s *r = w[0], *r0 = w[1], *p = w[2], *v = w[3], *s = w[4], *t = w[5];
    const int nbs = (c->geom.Vh + 63) / 64;                                     // workgroups (= partials) of one DOT hop on one parity: always one per 64-site chunk (the dot
                                                                                // instances have no multi-chunk / persistent form; stencil_num_blocks would say otherwise under dslash_pipe = 1 / 3)
    const int nbk = (int)std::min<size_t>(1024, (n + UB - 1) / UB);             // streaming kernels: at most 1024 partials (one prologue sums them)
    const bool fold = c->tun.bicg_fused >= 2 && nbs <= 1024;
    // bicg_fused = 4: the merged update launch on the two recurrences (bicgf_xrp_rec), <r0, t> from the second inner product of the dot epilogue
    const bool rec = c->tun.bicg_fused == 4;      // (every dot-mode kernel forms the second inner product: plain, clover-on-hop, scalar-addressing)
    c->tun.bicg_xrp_active = rec ? 2 : 0;
    double* P0 = c->d_partial;                  // <r0, v> (+ |v|^2)      [nbs x 3]
    double* P1 = P0 + (size_t)3 * nbs;          // |s|^2                  [nbk]
    double* P2 = P1 + nbk;                      // <t, s>, |t|^2          [nbs x 3]   (bicg_fused = 4: + <r0, t>, nbs x 5)
    double* P3 = P2 + (size_t)(rec ? 5 : 3) * nbs;   // |r|^2, <r0, r>    [nbk x 3]
    const bool soa = c->tun.bicg_dot_soa >= 2 || (c->tun.bicg_dot_soa == 1 && !fold && nbs > 1024);      // the dot partials of the hops as [value][workgroup] (tunable bicg_dot_soa)
    const double* skip_ = c->d_scal + (B_DONE - S_DONE);      // the kernels test skip[S_DONE]: the hops become no-ops once the solve is done
    auto schur = [&](lqcd_spinor_s* out, lqcd_spinor_s* in, const lqcd_spinor_s* z, double* dotp, int conj, bool skippable = true, const lqcd_spinor_s* z2 = nullptr) -> int {
        const double* skip = skippable ? skip_ : nullptr;
        StencilCall s1 = make_hop_call(op, to, in, nullptr, 0.0, 1.0, dg);      // t_o = [A_oo^-1] H_oe in
        s1.skip_flag = skip;
        if (Ai) { s1.clover = Ai; s1.clover_on_hop = 1; }
        LQCHK(stencil_apply(c, s1));
        StencilCall s2 = make_hop_call(op, out, to, in, 1.0, -k * k, dg);       // out = in - k^2 [A_ee^-1] H_eo t_o
        s2.skip_flag = skip;
        if (Ai) { s2.clover = Ai; s2.clover_on_hop = 1; }
        if (z) { s2.dot_z[0] = z->data; s2.dot_z[1] = nullptr; s2.dot_partial = dotp; s2.dot_conj = conj | (soa ? 2 : 0); }
        if (z2) { s2.dot_z2[0] = z2->data; s2.dot_z2[1] = nullptr; }
        return stencil_apply(c, s2);
    };
    // v = M x0 with hops that do not look at the done flag (the LAST solve left it raised), then r = rhs - v, r0 = p = r and the scalar block, all on the device
    const bool zero_guess = c->zero_guess_hint;      // the caller has just cleared x (the action / force solves): M x0 = 0 is not computed
    if (!zero_guess) LQCHK(schur(v, &xe, nullptr, nullptr, 0, false));
    hipLaunchKernelGGL(bicgf_init, dim3(nbk), dim3(UB), 0, c->stream, r->data, r0->data, p->data, rhs->data, zero_guess ? (const double2*)nullptr : (const double2*)v->data, n, P1);
    hipLaunchKernelGGL(bicgf_init_scal, dim3(1), dim3(64), 0, c->stream, P1, nbk, c->d_scal, eps);
    HIPCHK(hipGetLastError());
    (void)bytes;
    double rr = 0.0;
    int it = 0, st = LQCD_ERR_NOT_CONVERGED, enq = 0;
    bool breakdown = false;
    // Polling the done flag is a host round trip that idles the GPU for ~40 us: the first burst runs up to one iteration short of what the last
    // solve with this operator took (successive solves of an MD trajectory take the same count within one or two; iterations enqueued behind the
    // converging one are no-ops), later bursts are short.
    int check_every = std::max(4, std::min(op->bicg_hint, 64));      // (round 6: the last count itself -- a solve that takes it again is polled ONCE; one short made every solve pay two polls)
    while (st != LQCD_OK && !breakdown && it < maxiter) {
        const int burst = std::min(check_every, maxiter - it);
        check_every = 2;
        for (int q = 0; q < burst; q++, enq++) {
            BicgF a;
            a.sc = c->d_scal;
            a.fold = fold ? 1 : 0;
            a.rho_in = (enq & 1) ? B_RHOB : B_RHO;       // rho alternates between two slots: block 0 of the p update writes the next value while
            a.rho_out = (enq & 1) ? B_RHO : B_RHOB;      // the other workgroups still read this one
            a.pin2 = nullptr; a.pin2_n = 0;
            LQCHK(schur(v, p, r0, P0, 0));                                                                   // v = M p, <r0, v>
            if (!fold) LQCHK(reduce_to_slot(c, nbs, 3, B_R0V, true, 0, P0, soa));
            a.pin = P0; a.pin_n = nbs; a.pin_soa = soa ? 1 : 0; a.pout = P1;
            if (rec) { a.pin3 = P3; a.pin3_n = nbk; }
            hipLaunchKernelGGL(bicgf_s, dim3(nbk), dim3(UB), 0, c->stream, a, s->data, r->data, v->data, n);
            if (!fold && !rec) LQCHK(reduce_to_slot(c, nbk, 1, B_SS, true, 0, P1));      // (merged chain: the update launch sums the <= 1024 partials of |s|^2 itself)
            if (rec) {
                LQCHK(schur(t, s, s, P2, 1, true, r0));                                                      // t = M s, <t, s>, |t|^2, <r0, t>
                if (!fold) LQCHK(reduce_to_slot(c, nbs, 5, B_TS5, true, 0, P2, soa));
                a.pin = P2; a.pin_n = nbs; a.pin2 = P1; a.pin2_n = nbk; a.pout = P3;
                if (!fold) a.fold = 2;
                a.guard = std::pow(10.0, -(double)c->tun.bicg_rec_guard);
                hipLaunchKernelGGL(bicgf_xrp_rec, dim3(nbk), dim3(UB), 0, c->stream, a, xe.data, r->data, p->data, s->data, t->data, v->data, n);
                HIPCHK(hipGetLastError());
                continue;
            }
            LQCHK(schur(t, s, s, P2, 1));                                                                    // t = M s, <t, s>, |t|^2
            if (!fold) LQCHK(reduce_to_slot(c, nbs, 3, B_TS, true, 0, P2, soa));
            a.pin = P2; a.pin_n = nbs; a.pin2 = P1; a.pin2_n = nbk; a.pout = P3;
            hipLaunchKernelGGL(bicgf_xr, dim3(nbk), dim3(UB), 0, c->stream, a, xe.data, r->data, p->data, s->data, t->data, r0->data, n);
            if (!fold) LQCHK(reduce_to_slot(c, nbk, 3, B_RR, true, 0, P3));
            a.pin = P3; a.pin_n = nbk; a.pin_soa = 0; a.pin2 = nullptr; a.pin2_n = 0; a.pout = nullptr;
            hipLaunchKernelGGL(bicgf_p, dim3(nbk), dim3(UB), 0, c->stream, a, p->data, r->data, v->data, n);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(c->h_scal, c->d_scal + B_RHO, (B_END - B_RHO) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        it = (int)c->h_scal[B_ITERS - B_RHO];
        rr = c->h_scal[B_RES - B_RHO];
        const double done = c->h_scal[B_DONE - B_RHO];
        if (done == 1.0) st = LQCD_OK;
        else if (done != 0.0) breakdown = true;
    }
    if (iters) *iters = it;
    if (final_rr) *final_rr = rr;
    if (breakdown) { set_error("BiCGStab: residual is not finite (breakdown)"); return LQCD_ERR_NOT_CONVERGED; }
    if (st != LQCD_OK) {
        set_error("The BiCGStab is not converged! maxsteps = " + std::to_string(maxiter) + ", residual = " + std::to_string(rr));
        return LQCD_ERR_NOT_CONVERGED;
    }
    op->bicg_hint = it;
    return LQCD_OK;
}

}  // namespace lqcd

using namespace lqcd;

// even-odd (Schur) preconditioned BiCGStab, Wilson:
//   (1 - k^2 H_eo H_oe) x_e = b_e + k H_eo b_o ;  x_o = b_o + k H_oe x_e
// Wilson-clover (D_sw = A - k H, A block diagonal in parity): with the packed inverse blocks A^-1 (clover.hip)
//   (1 - k^2 A_ee^-1 H_eo A_oo^-1 H_oe) x_e = A_ee^-1 (b_e + k H_eo A_oo^-1 b_o) ;  x_o = A_oo^-1 (b_o + k H_oe x_e)
// (D_sw^+: H -> H^+ through the dagger flag of the hop, A is Hermitian).
extern "C" int lqcd_solve_bicgstab_eo(lqcd_op_t op, lqcd_spinor_t x, lqcd_spinor_t b, int dagger, double eps, int maxiter, int* iters,
                                      double* final_rr) {
    LQCHK(check_full(op, x, b, "lqcd_solve_bicgstab_eo"));
    ARGCHK(op->kind == LQCD_WILSON, "lqcd_solve_bicgstab_eo: Wilson only");
    lqcd_ctx_s* c = op->ctx;
    HIPCHK(hipSetDevice(c->device));
    apply_bc(c, op->bc);
    const bool clov = op->csw != 0.0 && op->clover;
    if (clov) {     // A follows the links, A^-1 follows A
        if (op->clover_version != op->gauge->version) {
            LQCHK(clover_build(c, op->gauge, op->clover, op->km, op->csw));
            op->clover_version = op->gauge->version;
        }
        if (!op->clover_inv) HIPCHK(hipMalloc((void**)&op->clover_inv, clover_elems(c->geom) * sizeof(double2)));
        if (op->clover_inv_version != op->clover_version) {
            LQCHK(clover_invert(c, op->clover, op->clover_inv));
            op->clover_inv_version = op->clover_version;
        }
    }
    const double2* Ai = op->clover_inv;
    const double k = op->km;
    const int dg = dagger ? 1 : 0;
    const size_t nh = x->elems / 2;
    ScratchScope pool(c);
    double2* wd[6];
    lqcd_spinor_s* wsp[6];
    for (int i = 0; i < 6; i++) {
        lqcd_spinor_s* wi = pool.get(op->kind, LQCD_EVEN);
        if (!wi) return LQCD_ERR_HIP;
        wd[i] = wi->data;
        wsp[i] = wi;
    }
    // plain Wilson r = 1 on an unpartitioned lattice: the chain whose inner products come from the Schur operator's epilogue (bicgstab_eo_wilson)
    const bool fused = c->tun.bicg_fused >= 1 && op->r == 1.0 && c->tun.dslash_variant == 1 && !any_partitioned(c) && !c->has_comm && c->geom.Vh % 64 == 0;
    lqcd_spinor_s* rhs = pool.get(op->kind, LQCD_EVEN);
    lqcd_spinor_s* te = clov ? pool.get(op->kind, LQCD_EVEN) : nullptr;
    lqcd_spinor_s* to = pool.get(op->kind, LQCD_ODD);
    lqcd_spinor_s* uo = clov ? pool.get(op->kind, LQCD_ODD) : nullptr;
    if (!rhs || !to || (clov && (!te || !uo))) return LQCD_ERR_HIP;
    // views of the even/odd halves of b and x
    lqcd_spinor_s be = *b, bo = *b, xe = *x, xo = *x;
    be.subset = xe.subset = LQCD_EVEN; bo.subset = xo.subset = LQCD_ODD;
    be.elems = bo.elems = xe.elems = xo.elems = nh;
    bo.data = b->data + nh; xo.data = x->data + nh;
    int st = LQCD_OK;
    auto run = [&]() -> int {
        lqcd_spinor_s vin = xe, vout = xe;
        ApplyFn A;
        if (!clov) {
            // rhs = b_e + k H_eo b_o
            { StencilCall s = make_hop_call(op, rhs, &bo, &be, 1.0, k, dg); LQCHK(stencil_apply(c, s)); }
            A = [&](double2* out, const double2* in) -> int {
                vin.data = const_cast<double2*>(in);
                vout.data = out;
                StencilCall s1 = make_hop_call(op, to, &vin, nullptr, 0.0, 1.0, dg);         // t_o = H_oe in
                LQCHK(stencil_apply(c, s1));
                StencilCall s2 = make_hop_call(op, &vout, to, &vin, 1.0, -k * k, dg);        // out = in - k^2 H_eo t_o
                return stencil_apply(c, s2);
            };
        } else {
            // rhs = A_ee^-1 (b_e + k H_eo A_oo^-1 b_o)
            LQCHK(clover_apply_parity(c, Ai, 1, uo->data, bo.data, 1.0, nullptr, 0.0));
            { StencilCall s = make_hop_call(op, te, uo, &be, 1.0, k, dg); LQCHK(stencil_apply(c, s)); }
            LQCHK(clover_apply_parity(c, Ai, 0, rhs->data, te->data, 1.0, nullptr, 0.0));
            A = [&](double2* out, const double2* in) -> int {
                vin.data = const_cast<double2*>(in);
                StencilCall s1 = make_hop_call(op, to, &vin, nullptr, 0.0, 1.0, dg);         // t_o = H_oe in
                LQCHK(stencil_apply(c, s1));
                LQCHK(clover_apply_parity(c, Ai, 1, uo->data, to->data, 1.0, nullptr, 0.0)); // u_o = A_oo^-1 t_o
                StencilCall s2 = make_hop_call(op, te, uo, nullptr, 0.0, 1.0, dg);           // t_e = H_eo u_o
                LQCHK(stencil_apply(c, s2));
                return clover_apply_parity(c, Ai, 0, out, te->data, -k * k, in, 1.0);        // out = in - k^2 A_ee^-1 t_e
            };
        }
        const bool mixed = fused && c->tun.bicg_mixed;                // fp32 inner chain, fp64 defect correction (mixed.hip); same contract
        const int sc = mixed ? bicgstab_eo_wilson_mixed(op, xe, rhs, wsp, to, dg, eps, maxiter, iters, final_rr, clov ? Ai : nullptr)
                     : fused ? bicgstab_eo_wilson(op, xe, rhs, wsp, to, dg, eps, maxiter, iters, final_rr, clov ? Ai : nullptr)
                             : bicgstab_core(c, A, nh, xe.data, rhs->data, wd, eps, maxiter, iters, final_rr);
        // the odd half (also on non-convergence, so x is a consistent best effort)
        if (!clov) {
            StencilCall s = make_hop_call(op, &xo, &xe, &bo, 1.0, k, dg);                    // x_o = b_o + k H_oe x_e
            LQCHK(stencil_apply(c, s));
        } else {
            StencilCall s = make_hop_call(op, to, &xe, &bo, 1.0, k, dg);
            LQCHK(stencil_apply(c, s));
            LQCHK(clover_apply_parity(c, Ai, 1, xo.data, to->data, 1.0, nullptr, 0.0));      // x_o = A_oo^-1 (b_o + k H_oe x_e)
        }
        return sc;
    };
    st = run();
    hipError_t e = hipStreamSynchronize(c->stream);      // before the scratch fields go back to the pool
    if (st == LQCD_OK && e != hipSuccess) st = hip_fail(e, "sync bicgstab_eo", __FILE__, __LINE__);
    return st;
}
