// bicgstab.hip -- BiCGStab with device-resident scalars on an operator given as an enqueue function, and the host-scalar BiCG.
//
// Replaces, behind the C ABI, LatticeDiracOperators.jl's solve_DinvX!(y, D | D', x) (bicgstab / bicg) -- SURVEY.md 8(a) a5.
#include "ops_internal.h"

#include <algorithm>
#include <cmath>
#include <complex>

namespace lqcd {

// ---------------------------------------------------------------------------------- BiCGStab (device-resident scalars)
// One iteration = 2 operator applications + 5 streaming kernels + 4 single-block reductions, all enqueued without a host
// round trip; complex alpha/omega/beta live in d_scal[B_*] (scalar steps: blas.hip cg_scalar_step ops 3..6).  The host
// polls the done flag every few iterations.  Same recurrences, stopping rule (|s|^2 < eps half-step exit, |r|^2 < eps) and
// iteration count as the textbook van der Vorst loop the parity tests compare against.

// <a,b> = sum conj(a) b
__global__ __launch_bounds__(UB) void bicg_dot(const double* __restrict__ sc, const double2* __restrict__ a, const double2* __restrict__ b, size_t n,
                                                double* partial) {
    if (sc[B_DONE] != 0.0) return;
    double acc[2] = {0, 0};
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        const double2 x = a[i], y = b[i];
        acc[0] = fma(x.x, y.x, acc[0]); acc[0] = fma(x.y, y.y, acc[0]);
        acc[1] = fma(x.x, y.y, acc[1]); acc[1] = fma(-x.y, y.x, acc[1]);
    }
    block_reduce_nv<2>(acc, partial);
}
// s = r - alpha v ; partial |s|^2
__global__ __launch_bounds__(UB) void bicg_s(const double* __restrict__ sc, double2* __restrict__ s, const double2* __restrict__ r,
                                              const double2* __restrict__ v, size_t n, double* partial) {
    if (sc[B_DONE] != 0.0) return;
    const double ar = sc[B_ALPHA], ai = sc[B_ALPHA + 1];
    double acc[1] = {0};
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        const double2 vv = v[i];
        double2 sv = r[i];
        sv.x = fma(-ar, vv.x, sv.x); sv.x = fma(ai, vv.y, sv.x);
        sv.y = fma(-ar, vv.y, sv.y); sv.y = fma(-ai, vv.x, sv.y);
        s[i] = sv;
        acc[0] = fma(sv.x, sv.x, acc[0]); acc[0] = fma(sv.y, sv.y, acc[0]);
    }
    block_reduce_nv<1>(acc, partial);
}
// partials of <t,s> (2 values) and |t|^2
__global__ __launch_bounds__(UB) void bicg_ts(const double* __restrict__ sc, const double2* __restrict__ t, const double2* __restrict__ s, size_t n,
                                               double* partial) {
    if (sc[B_DONE] != 0.0) return;
    double acc[3] = {0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        const double2 x = t[i], y = s[i];
        acc[0] = fma(x.x, y.x, acc[0]); acc[0] = fma(x.y, y.y, acc[0]);
        acc[1] = fma(x.x, y.y, acc[1]); acc[1] = fma(-x.y, y.x, acc[1]);
        acc[2] = fma(x.x, x.x, acc[2]); acc[2] = fma(x.y, x.y, acc[2]);
    }
    block_reduce_nv<3>(acc, partial);
}
// x += alpha p + omega s ; r = s - omega t ; partials |r|^2, <r0,r>
__global__ __launch_bounds__(UB) void bicg_xr(const double* __restrict__ sc, double2* __restrict__ x, double2* __restrict__ r,
                                               const double2* __restrict__ p, const double2* __restrict__ s, const double2* __restrict__ t,
                                               const double2* __restrict__ r0, size_t n, double* partial) {
    if (sc[B_DONE] != 0.0) return;
    const double ar = sc[B_ALPHA], ai = sc[B_ALPHA + 1], wr = sc[B_OMEGA], wi = sc[B_OMEGA + 1];
    double acc[3] = {0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        const double2 pv = p[i], sv = s[i], tv = t[i], zv = r0[i];
        double2 xv = x[i], rv = sv;
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
    }
    block_reduce_nv<3>(acc, partial);
}
// p = r + beta (p - omega v)
__global__ __launch_bounds__(UB) void bicg_p(const double* __restrict__ sc, double2* __restrict__ p, const double2* __restrict__ r,
                                              const double2* __restrict__ v, size_t n) {
    if (sc[B_DONE] != 0.0) return;
    const double br = sc[B_BETA], bi = sc[B_BETA + 1], wr = sc[B_OMEGA], wi = sc[B_OMEGA + 1];
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        const double2 vv = v[i], rv = r[i];
        double2 pv = p[i];
        pv.x = fma(-wr, vv.x, pv.x); pv.x = fma(wi, vv.y, pv.x);
        pv.y = fma(-wr, vv.y, pv.y); pv.y = fma(-wi, vv.x, pv.y);
        double2 o;
        o.x = fma(br, pv.x, rv.x); o.x = fma(-bi, pv.y, o.x);
        o.y = fma(br, pv.y, rv.y); o.y = fma(bi, pv.x, o.y);
        p[i] = o;
    }
}

int bicgstab_core(lqcd_ctx_s* c, const ApplyFn& A, size_t n, double2* x, const double2* b, double2* const w[6], double eps,
                  int maxiter, int* iters, double* final_rr) {
    double2 *r = w[0], *r0 = w[1], *p = w[2], *v = w[3], *s = w[4], *t = w[5];
    const size_t bytes = n * sizeof(double2);
    LQCHK(A(v, x));
    HIPCHK(hipMemcpyAsync(r, b, bytes, hipMemcpyDeviceToDevice, c->stream));
    LQCHK(blas_axpy(c, -1.0, 0.0, v, r, n));
    HIPCHK(hipMemcpyAsync(r0, r, bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(p, r, bytes, hipMemcpyDeviceToDevice, c->stream));
    double rr;
    LQCHK(blas_norm2(c, r, n, &rr, true));
    double init[B_END - B_RHO] = {0};
    init[B_RHO - B_RHO] = rr;
    init[B_EPS - B_RHO] = eps;
    init[B_RES - B_RHO] = rr;
    HIPCHK(hipMemcpyAsync(c->d_scal + B_RHO, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int it = 0, st = LQCD_ERR_NOT_CONVERGED;
    bool breakdown = false;
    if (rr < eps) st = LQCD_OK;
    const int nb = stream_grid(c, n), check_every = 4;
    const double* sc = c->d_scal;
    while (st != LQCD_OK && !breakdown && it < maxiter) {
        const int burst = std::min(check_every, maxiter - it);
        for (int k = 0; k < burst; k++) {
            LQCHK(A(v, p));
            hipLaunchKernelGGL(bicg_dot, dim3(nb), dim3(UB), 0, c->stream, sc, r0, v, n, c->d_partial);
            LQCHK(reduce_to_slot(c, nb, 2, B_R0V, true, 3));
            hipLaunchKernelGGL(bicg_s, dim3(nb), dim3(UB), 0, c->stream, sc, s, r, v, n, c->d_partial);
            LQCHK(reduce_to_slot(c, nb, 1, B_SS, true, 4));
            LQCHK(A(t, s));
            hipLaunchKernelGGL(bicg_ts, dim3(nb), dim3(UB), 0, c->stream, sc, t, s, n, c->d_partial);
            LQCHK(reduce_to_slot(c, nb, 3, B_TS, true, 5));
            hipLaunchKernelGGL(bicg_xr, dim3(nb), dim3(UB), 0, c->stream, sc, x, r, p, s, t, r0, n, c->d_partial);
            LQCHK(reduce_to_slot(c, nb, 3, B_RR, true, 6));
            hipLaunchKernelGGL(bicg_p, dim3(nb), dim3(UB), 0, c->stream, sc, p, r, v, n);
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
    return LQCD_OK;
}

}  // namespace lqcd

using namespace lqcd;

extern "C" int lqcd_solve_bicgstab(lqcd_op_t op, lqcd_spinor_t x, lqcd_spinor_t b, int dagger, double eps, int maxiter, int* iters,
                                   double* final_rr) {
    LQCHK(check_full(op, x, b, "lqcd_solve_bicgstab"));
    lqcd_ctx_s* c = op->ctx;
    HIPCHK(hipSetDevice(c->device));
    ScratchScope pool(c);
    double2* wd[6];
    for (int i = 0; i < 6; i++) {
        lqcd_spinor_s* wi = pool.get(op->kind, LQCD_FULL);
        if (!wi) return LQCD_ERR_HIP;
        wd[i] = wi->data;
    }
    // the stencil works on spinor handles; wrap raw pointers of the scratch fields
    lqcd_spinor_s vin = *x, vout = *x;
    ApplyFn A = [&](double2* out, const double2* in) -> int {
        vin.data = const_cast<double2*>(in);
        vout.data = out;
        return op_apply_async(op, &vout, &vin, dagger ? 1 : 0, nullptr);
    };
    return bicgstab_core(c, A, x->elems, x->data, b->data, wd, eps, maxiter, iters, final_rr);
}

// BiCG (`bicg`, the default method_CG of solve_DinvX!(y, D, x): SURVEY.md 3.3): coupled recurrences with A and A^+, shadow residual
// r~_0 = r_0, stopping rule real(r.r) < eps.  Offered for completeness of the reference's solver list: the scalars go through the host
// (three synchronising reductions per iteration); the hot paths use the device-scalar CG / BiCGStab above.  x holds the initial guess.
extern "C" int lqcd_solve_bicg(lqcd_op_t op, lqcd_spinor_t x, lqcd_spinor_t b, int dagger, double eps, int maxiter, int* iters, double* final_rr) {
    LQCHK(check_full(op, x, b, "lqcd_solve_bicg"));
    ARGCHK(maxiter >= 0, "lqcd_solve_bicg: maxiter < 0");
    lqcd_ctx_s* c = op->ctx;
    HIPCHK(hipSetDevice(c->device));
    ScratchScope pool(c);
    lqcd_spinor_s* w[6];
    for (auto& f : w) { f = pool.get(op->kind, LQCD_FULL); if (!f) return LQCD_ERR_HIP; }
    lqcd_spinor_s *r = w[0], *rt = w[1], *p = w[2], *pt = w[3], *q = w[4], *qt = w[5];
    const size_t n = x->elems, bytes = n * sizeof(double2);
    const int dg = dagger ? 1 : 0;
    LQCHK(op_apply_async(op, q, x, dg, nullptr));
    HIPCHK(hipMemcpyAsync(r->data, b->data, bytes, hipMemcpyDeviceToDevice, c->stream));
    LQCHK(blas_axpy(c, -1.0, 0.0, q->data, r->data, n));
    for (lqcd_spinor_s* f : {rt, p, pt}) HIPCHK(hipMemcpyAsync(f->data, r->data, bytes, hipMemcpyDeviceToDevice, c->stream));
    double rr = 0, im = 0;
    LQCHK(blas_norm2(c, r->data, n, &rr, true));
    std::complex<double> rho(rr, 0.0);      // <r~, r> with r~ = r
    int it = 0;
    bool converged = rr < eps;
    while (!converged && it < maxiter) {
        it++;
        LQCHK(op_apply_async(op, q, p, dg, nullptr));
        LQCHK(op_apply_async(op, qt, pt, 1 - dg, nullptr));
        double dr = 0, di = 0;
        LQCHK(blas_dot(c, pt->data, q->data, n, &dr, &di, true));
        const std::complex<double> alpha = rho / std::complex<double>(dr, di);
        if (!std::isfinite(alpha.real()) || !std::isfinite(alpha.imag())) { set_error("BiCG: breakdown (<p~, A p> = 0)"); return LQCD_ERR_NOT_CONVERGED; }
        LQCHK(blas_axpy(c, alpha.real(), alpha.imag(), p->data, x->data, n));
        LQCHK(blas_axpy(c, -alpha.real(), -alpha.imag(), q->data, r->data, n));
        LQCHK(blas_axpy(c, -alpha.real(), alpha.imag(), qt->data, rt->data, n));        // r~ -= conj(alpha) A^+ p~
        LQCHK(blas_norm2(c, r->data, n, &rr, true));
        if (rr < eps) { converged = true; break; }
        LQCHK(blas_dot(c, rt->data, r->data, n, &dr, &im, true));
        const std::complex<double> rho1(dr, im), beta = rho1 / rho;
        LQCHK(blas_axpby(c, 1.0, 0.0, r->data, beta.real(), beta.imag(), p->data, n));          // p = r + beta p
        LQCHK(blas_axpby(c, 1.0, 0.0, rt->data, beta.real(), -beta.imag(), pt->data, n));       // p~ = r~ + conj(beta) p~
        rho = rho1;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (iters) *iters = it;
    if (final_rr) *final_rr = rr;
    if (!converged) {
        set_error("The BiCG is not converged! maxsteps = " + std::to_string(maxiter) + ", residual = " + std::to_string(rr));
        return LQCD_ERR_NOT_CONVERGED;
    }
    return LQCD_OK;
}
