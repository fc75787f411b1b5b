// multishift.hip -- multi-shift CG on D^+D + sigma_j (the solver of the RHMC path): zeta recurrences on the device next to the CG scalars.
//
// Replaces, behind the C ABI, LatticeDiracOperators.jl's shiftedcg -- SURVEY.md 8(f) rank 3.
#include "ops_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace lqcd;

// ---------------------------------------------------------------------------------- multi-shift CG (RHMC solver)
namespace lqcd {
// per-shift coefficient block in device memory: [sigma | zeta_{n-1} | zeta_n | a | b | z] (ns doubles each), alpha_{n-1}, beta_{n-1}
// zeta recurrence (Jegerlehner hep-lat/9612014) after the base system's alpha_n, beta_n are known:
//   zeta_{n+1} = zeta_n zeta_{n-1} alpha_{n-1} / (zeta_{n-1} alpha_{n-1} (1 + alpha_n sigma) + alpha_n beta_{n-1} (zeta_{n-1} - zeta_n))
//   x_j += (zeta_{n+1}/zeta_n) alpha_n p_j ;  p_j = (zeta_{n+1}/zeta_n)^2 beta_n p_j + zeta_{n+1} r
// stop_when_frozen: the base system only drives the Krylov space (no unshifted solution is wanted): once every shift is frozen the
// solve is complete -- S_DONE is raised here, the update kernel behind this launch applies the last x_j steps, later launches are no-ops.
__global__ void ms_zeta(double* __restrict__ sc, double* __restrict__ ms, int ns, int stop_when_frozen) {
    __shared__ int active;
    if (threadIdx.x == 0) active = 0;
    __syncthreads();
    if (sc[S_XDONE] != 0.0) return;
    const double alpha = sc[S_ALPHA], beta = sc[S_BETA], alpha_m = ms[6 * ns], beta_m = ms[6 * ns + 1];
    for (int j = threadIdx.x; j < ns; j += blockDim.x) {
        const double sigma = ms[j], zm = ms[ns + j], z0 = ms[2 * ns + j];
        if (fabs(z0) < 1e-100) {      // this shift converged long ago (its residual is zeta^2 |r|^2): freeze it before zeta underflows to 0/0
            ms[3 * ns + j] = 0.0; ms[4 * ns + j] = 0.0; ms[5 * ns + j] = 0.0;
            continue;
        }
        const double den = zm * alpha_m * (1.0 + alpha * sigma) + alpha * beta_m * (zm - z0);
        const double zp = z0 * zm * alpha_m / den, ratio = zp / z0;
        ms[3 * ns + j] = ratio * alpha;
        if (zp * zp * sc[S_RR] < sc[S_EPS]) {
            // the residual of this shift, zeta^2 |r|^2, is below the target once x_j has taken this step: last update, then the
            // shift is frozen (p_j = 0, no further traffic) -- large shifts drop out after a few tens of iterations
            ms[4 * ns + j] = 0.0; ms[5 * ns + j] = 0.0; ms[ns + j] = 0.0; ms[2 * ns + j] = 0.0;
            continue;
        }
        ms[4 * ns + j] = ratio * ratio * beta;
        ms[5 * ns + j] = zp;
        ms[ns + j] = z0;
        ms[2 * ns + j] = zp;
        active = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ms[6 * ns] = alpha; ms[6 * ns + 1] = beta;
        if (stop_when_frozen && !active) sc[S_DONE] = 1.0;
    }
}
int ms_zeta_launch(lqcd_ctx_s* c, double* d_ms, int ns, int stop_when_frozen) {
    hipLaunchKernelGGL(ms_zeta, dim3(1), dim3(64), 0, c->stream, c->d_scal, d_ms, ns, stop_when_frozen);
    HIPCHK(hipGetLastError());
    return LQCD_OK;
}
// base system (x += alpha p ; p = r + beta p) and every active shifted system j (x_j += a_j p_j ; p_j = b_j p_j + z_j r) in one pass:
// r is read once per element, frozen shifts cost nothing.  x is still updated in the iteration that converges; nothing is touched
// afterwards.
// NT (tunable nt_blas): the shifted x_j, p_j are streamed -- an element is not touched again before 2 x (active shifts) fields have gone by
template <bool NT>
__global__ __launch_bounds__(UB) void ms_update_all(const double* __restrict__ sc, const double* __restrict__ ms, double2* const* __restrict__ ptr,
                                                     double2* __restrict__ x0, double2* __restrict__ p0, const double2* __restrict__ r, size_t n,
                                                     int ns) {
    if (sc[S_XDONE] != 0.0) return;
    const double al = sc[S_ALPHA], be = sc[S_BETA];
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        const double2 rv = r[i];
        {
            double2 pv = p0[i];
            if (x0) {          // the unshifted solution is optional (a rational action only wants the shifted ones)
                double2 xv = ldx<NT>(x0 + i);
                xv.x = fma(al, pv.x, xv.x); xv.y = fma(al, pv.y, xv.y);
                stx<NT>(x0 + i, xv);
            }
            pv.x = fma(be, pv.x, rv.x); pv.y = fma(be, pv.y, rv.y);
            p0[i] = pv;
        }
        for (int j = 0; j < ns; j++) {
            const double a = ms[3 * ns + j], bb = ms[4 * ns + j], z = ms[5 * ns + j];
            if (a == 0.0 && bb == 0.0 && z == 0.0) continue;       // frozen shift
            double2* __restrict__ x = ptr[j];
            double2* __restrict__ p = ptr[ns + j];
            double2 pv = ldx<NT>(p + i), xv = ldx<NT>(x + i);
            xv.x = fma(a, pv.x, xv.x); xv.y = fma(a, pv.y, xv.y);
            pv.x = fma(bb, pv.x, z * rv.x); pv.y = fma(bb, pv.y, z * rv.y);
            stx<NT>(x + i, xv); stx<NT>(p + i, pv);
        }
    }
}
}  // namespace lqcd

// (D^+D + sigma_j) x_j = b for all j < ns, plus the unshifted solution x0 (may be NULL): one Krylov space, the shifted
// iterates follow from the zeta recurrences, which run on the device next to the CG scalars (no host round trip inside an
// iteration; the host polls the convergence flag every 8 iterations).  Zero initial guesses.  Stops when |r|^2 < eps
// (for sigma_j >= 0 every |zeta_j| <= 1, so the shifted residuals zeta_j r are then below eps as well).
extern "C" int lqcd_solve_multishift_cg(lqcd_op_t op, lqcd_spinor_t x0, lqcd_spinor_t* xs, lqcd_spinor_t b, const double* sigma, int ns,
                                        double eps, int maxiter, int* iters, double* final_rr) {
    LQCHK(lqcd::links_flush_of(op));      // recorded single-direction link operations run first (links.hip)
    ARGCHK(op && b && ns >= 0 && ns <= 1024 && (ns == 0 || (xs && sigma)), "lqcd_solve_multishift_cg: null argument or more than 1024 shifts");
    ARGCHK(b->ctx == op->ctx && b->kind == op->kind && b->subset == LQCD_FULL, "lqcd_solve_multishift_cg: b must be a FULL spinor of the operator");
    for (int j = 0; j < ns; j++) {
        ARGCHK(xs[j] && xs[j]->ctx == op->ctx && xs[j]->kind == op->kind && xs[j]->subset == LQCD_FULL && xs[j] != b,
               "lqcd_solve_multishift_cg: xs[j] must be distinct FULL spinors of the operator");
        ARGCHK(sigma[j] >= 0.0, "lqcd_solve_multishift_cg: shifts must be non-negative");
        ARGCHK(xs[j] != x0, "lqcd_solve_multishift_cg: xs[j] and x0 must be different fields (every system is updated in place on its own handle)");
        for (int i = 0; i < j; i++) ARGCHK(xs[i] != xs[j], "lqcd_solve_multishift_cg: the xs[j] must be pairwise different fields");
    }
    if (x0) LQCHK(check_full(op, x0, b, "lqcd_solve_multishift_cg"));
    lqcd_ctx_s* c = op->ctx;
    HIPCHK(hipSetDevice(c->device));
    const size_t n = b->elems, bytes = n * sizeof(double2);
    lqcd_spinor_s* xbase = x0;          // may stay null: then the base system only drives the Krylov space
    lqcd_spinor_s* r = scratch_get(c, op->kind, LQCD_FULL);
    lqcd_spinor_s* p = scratch_get(c, op->kind, LQCD_FULL);
    lqcd_spinor_s* q = scratch_get(c, op->kind, LQCD_FULL);
    lqcd_spinor_s* tmp = scratch_get(c, op->kind, LQCD_FULL);
    std::vector<lqcd_spinor_s*> ps(ns, nullptr);
    bool ok = r && p && q && tmp;
    for (int j = 0; j < ns && ok; j++) { ps[j] = scratch_get(c, op->kind, LQCD_FULL); ok = ps[j] != nullptr; }
    const size_t ms_doubles = 6 * (size_t)ns + 2, ms_bytes = ms_doubles * sizeof(double) + 2 * (size_t)ns * sizeof(double2*);
    char* d_blk = nullptr;
    if (ok && hipMalloc((void**)&d_blk, ms_bytes) != hipSuccess) ok = false;
    auto release = [&]() {
        scratch_put(r); scratch_put(p); scratch_put(q); scratch_put(tmp);
        for (auto* s : ps) scratch_put(s);
        if (d_blk) (void)hipFree(d_blk);
    };
    if (!ok) { release(); set_error("lqcd_solve_multishift_cg: out of device memory"); return LQCD_ERR_HIP; }
    double* d_ms = (double*)d_blk;
    double2** d_ptr = (double2**)(d_blk + ms_doubles * sizeof(double));
    auto run = [&]() -> int {
        if (xbase) HIPCHK(hipMemsetAsync(xbase->data, 0, bytes, c->stream));
        HIPCHK(hipMemcpyAsync(r->data, b->data, bytes, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(p->data, b->data, bytes, hipMemcpyDeviceToDevice, c->stream));
        std::vector<double> hms(ms_doubles, 1.0);    // zeta_{-1} = zeta_0 = 1, alpha_{-1} = 1
        std::vector<double2*> hptr(2 * (size_t)ns);
        for (int j = 0; j < ns; j++) {
            HIPCHK(hipMemsetAsync(xs[j]->data, 0, bytes, c->stream));
            HIPCHK(hipMemcpyAsync(ps[j]->data, b->data, bytes, hipMemcpyDeviceToDevice, c->stream));
            hms[j] = sigma[j];
            hptr[j] = xs[j]->data;
            hptr[ns + j] = ps[j]->data;
        }
        hms[6 * (size_t)ns + 1] = 0.0;               // beta_{-1} = 0
        HIPCHK(hipMemcpyAsync(d_ms, hms.data(), ms_doubles * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (ns) HIPCHK(hipMemcpyAsync(d_ptr, hptr.data(), 2 * (size_t)ns * sizeof(double2*), hipMemcpyHostToDevice, c->stream));
        double rr = 0.0;
        LQCHK(blas_norm2(c, r->data, n, &rr, true));
        double init[9] = {rr, 0, 0, 0, 0, 0, eps, 0, 0};   // S_RR .. S_XDONE
        HIPCHK(hipMemcpyAsync(c->d_scal + S_RR, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        int it = 0;
        bool converged = rr < eps;
        LQCHK(halo_schedule_settle(op));
        const int nbs = stencil_num_partials(c, op->kind, op->r, 2, 0, op_fused_clover(op)), nbu = stream_grid(c, n), check_every = 8;
        while (!converged && it < maxiter) {
            const int burst = std::min(check_every, maxiter - it);
            for (int k = 0; k < burst; k++) {
                // tmp = D p, alpha = rr / |tmp|^2 ; r -= alpha D^+ tmp in the stencil epilogue, beta = rr'/rr
                LQCHK(op_apply_async(op, tmp, p, 0, c->d_partial, c->d_scal));
                LQCHK(reduce_to_slot(c, nbs, 1, S_PQ, true, 1));
                apply_bc(c, op->bc);
                StencilCall s2;
                LQCHK(make_full_call(op, q, tmp, 1, s2));
                s2.norm_partial = c->d_partial;
                s2.upd_scal = c->d_scal;
                s2.upd[0] = spinor_block(r, 0);
                s2.upd[1] = spinor_block(r, 1);
                LQCHK(stencil_apply(c, s2));
                LQCHK(reduce_to_slot(c, nbs, 1, S_RRNEW, true, 2));
                if (ns) LQCHK(ms_zeta_launch(c, d_ms, ns, 0));
                if (c->tun.nt_blas) hipLaunchKernelGGL(ms_update_all<true>, dim3(nbu), dim3(UB), 0, c->stream, c->d_scal, d_ms, d_ptr, xbase ? xbase->data : (double2*)nullptr, p->data,
                                   r->data, n, ns);
                else hipLaunchKernelGGL(ms_update_all<false>, dim3(nbu), dim3(UB), 0, c->stream, c->d_scal, d_ms, d_ptr, xbase ? xbase->data : (double2*)nullptr, p->data,
                                   r->data, n, ns);
                HIPCHK(hipGetLastError());
            }
            HIPCHK(hipMemcpyAsync(c->h_scal, c->d_scal + S_RR, 8 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            rr = c->h_scal[S_RR - S_RR];
            it = (int)c->h_scal[S_ITERS - S_RR];
            if (c->h_scal[S_DONE - S_RR] != 0.0) converged = true;
            if (!std::isfinite(rr)) { set_error("multi-shift CG: residual is not finite"); break; }
        }
        if (iters) *iters = it;
        if (final_rr) *final_rr = rr;
        if (!converged) {
            if (std::isfinite(rr))
                set_error("The shifted CG is not converged! maxsteps = " + std::to_string(maxiter) + ", residual = " + std::to_string(rr));
            return LQCD_ERR_NOT_CONVERGED;
        }
        return LQCD_OK;
    };
    const int st = run();
    (void)hipStreamSynchronize(c->stream);
    release();
    return st;
}
