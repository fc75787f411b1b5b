// bicgstab_eo_mrhs.hip -- several right-hand sides: the multi-column hop / operator entries and the even-odd BiCGStab of the plain Wilson operator batched over columns.
//
// The solver is bicgstab_eo_wilson (bicgstab_eo.hip) with a column index: the same recurrences and the same stopping rule (half-step exit on |s|^2 < eps, then
// |r|^2 < eps, absolute), applied per column.  Every column has its own Krylov scalars and its own done flag in a per-context device block of
// n x (B_END - B_RHO) doubles (slot B_x of column j at blk[j * MR_NS + B_x - B_RHO]).  One iteration for all columns, the unfolded form:
//     multi-hop, multi-hop + <r0, v>          v = M p                      (stencil_mrhs.hip; M = 1 - k^2 H_eo H_oe)
//     mr_step_alpha                           alpha = rho / <r0, v>
//     mr_s                                    s = r - alpha v, |s|^2 partials
//     multi-hop, multi-hop + <t, s>, |t|^2    t = M s
//     mr_step_omega                           half-step test on |s|^2, omega = <t, s> / |t|^2
//     mr_xr                                   x += alpha p + omega s, r = s - omega t, |r|^2 and <r0, r> partials
//     mr_step_beta                            iteration count, convergence / breakdown, beta, rho = rho'
//     mr_p                                    p = r + beta (p - omega v)
// The streaming kernels take the column as blockIdx.y, the step kernels as blockIdx.x (one workgroup sums a column's partials in a fixed order).  A done flag is
// written by the step kernels alone, never by a launch that tests it at entry in other workgroups (B_DONE): a converged column is frozen -- nothing of it
// is read or written by later iterations and its count stops.  The host polls once per burst with one copy of all columns' blocks.
#include "ops_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace lqcd {

constexpr int MR_NS = B_END - B_RHO;      // doubles per column
constexpr int MR_RB = 1024;               // threads of a step kernel
__host__ __device__ constexpr int mb(int slot) { return slot - B_RHO; }

struct MrVec {      // the work vectors of every column (even half-fields)
    double2* x[LQCD_MRHS_MAX];
    double2* r[LQCD_MRHS_MAX];
    double2* r0[LQCD_MRHS_MAX];
    double2* p[LQCD_MRHS_MAX];
    double2* v[LQCD_MRHS_MAX];
    double2* s[LQCD_MRHS_MAX];
    double2* t[LQCD_MRHS_MAX];
    const double2* rhs[LQCD_MRHS_MAX];
};
struct MrBuf {      // the per-context block: scalars, then the partial sums of every column
    double* sc;     // [n][MR_NS]
    double* P0;     // <r0, v>            [n][nbs x 3]
    double* P1;     // |s|^2              [n][nbk]
    double* P2;     // <t, s>, |t|^2      [n][nbs x 3]
    double* P3;     // |r|^2, <r0, r>     [n][nbk x 3]
    int nbs, nbk;
};
// entry j of a table held in kernel arguments without a dynamic index (which would send the argument struct through scratch)
template <typename T>
__device__ __forceinline__ T pick12(T const (&t)[LQCD_MRHS_MAX], int j) {
    T p = t[0];
#pragma unroll
    for (int q = 1; q < LQCD_MRHS_MAX; q++) p = j == q ? t[q] : p;
    return p;
}

// sum of value v of nb partials [block][nv], the same order whatever the grid that wrote them: thread t adds partials t, t + 1024, ... in sequence, the 64 sums of a
// wave go through the DPP tree, the 16 wave sums are added in sequence.  The result is valid in thread 0.
__device__ inline double mr_block_sum(const double* __restrict__ partial, int nb, int nv, int v) {
    __shared__ double ws[MR_RB / 64];
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += MR_RB) a += partial[(size_t)i * nv + v];
    a = wave_sum(a);
    __syncthreads();      // (ws may still be read by thread 0 for the value before)
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = a;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int q = 0; q < MR_RB / 64; q++) s += ws[q];
    return s;
}

// ---------------------------------------------------------------------------------- step kernels: one workgroup per column
__global__ __launch_bounds__(MR_RB) void mr_init_scal(MrBuf b, double eps) {
    double* sc = b.sc + (size_t)blockIdx.x * MR_NS;
    const double rr = mr_block_sum(b.P1 + (size_t)blockIdx.x * b.nbk, b.nbk, 1, 0);
    if (threadIdx.x == 0) {
        for (int j = 0; j < MR_NS; j++) sc[j] = 0.0;
        sc[mb(B_RHO)] = rr; sc[mb(B_EPS)] = eps; sc[mb(B_RES)] = rr;
        if (rr < eps) sc[mb(B_DONE)] = 1.0;
        else if (!(fabs(rr) <= 1.79e308)) sc[mb(B_DONE)] = 2.0;
    }
}
__global__ __launch_bounds__(MR_RB) void mr_step_alpha(MrBuf b) {
    double* sc = b.sc + (size_t)blockIdx.x * MR_NS;
    if (sc[mb(B_DONE)] != 0.0) return;
    const double* P = b.P0 + (size_t)blockIdx.x * 3 * b.nbs;
    c2 r0v;
    r0v.re = mr_block_sum(P, b.nbs, 3, 0);
    r0v.im = mr_block_sum(P, b.nbs, 3, 1);
    if (threadIdx.x == 0) {
        const c2 rho = {sc[mb(B_RHO)], sc[mb(B_RHO) + 1]};
        const c2 al = bicg_alpha(rho, r0v);
        sc[mb(B_R0V)] = r0v.re; sc[mb(B_R0V) + 1] = r0v.im; sc[mb(B_ALPHA)] = al.re; sc[mb(B_ALPHA) + 1] = al.im;
    }
}
__global__ __launch_bounds__(MR_RB) void mr_step_omega(MrBuf b) {
    double* sc = b.sc + (size_t)blockIdx.x * MR_NS;
    if (sc[mb(B_DONE)] != 0.0) return;
    const double* P = b.P2 + (size_t)blockIdx.x * 3 * b.nbs;
    const double ss = mr_block_sum(b.P1 + (size_t)blockIdx.x * b.nbk, b.nbk, 1, 0);
    c2 ts;
    ts.re = mr_block_sum(P, b.nbs, 3, 0);
    ts.im = mr_block_sum(P, b.nbs, 3, 1);
    const double tt = mr_block_sum(P, b.nbs, 3, 2);
    if (threadIdx.x == 0) {
        const bool half = ss < sc[mb(B_EPS)];
        const c2 om = bicg_omega(ts, tt, half);
        sc[mb(B_SS)] = ss; sc[mb(B_HALF)] = half ? 1.0 : 0.0; sc[mb(B_TS)] = ts.re; sc[mb(B_TS) + 1] = ts.im; sc[mb(B_TT)] = tt;
        sc[mb(B_OMEGA)] = om.re; sc[mb(B_OMEGA) + 1] = om.im;
    }
}
__global__ __launch_bounds__(MR_RB) void mr_step_beta(MrBuf b) {
    double* sc = b.sc + (size_t)blockIdx.x * MR_NS;
    if (sc[mb(B_DONE)] != 0.0) return;
    const double* P = b.P3 + (size_t)blockIdx.x * 3 * b.nbk;
    const double rrn = mr_block_sum(P, b.nbk, 3, 0);
    c2 rho1;
    rho1.re = mr_block_sum(P, b.nbk, 3, 1);
    rho1.im = mr_block_sum(P, b.nbk, 3, 2);
    if (threadIdx.x == 0) {
        const bool half = sc[mb(B_HALF)] != 0.0;
        const double rr = half ? sc[mb(B_SS)] : rrn;
        sc[mb(B_ITERS)] += 1.0; sc[mb(B_RES)] = rr; sc[mb(B_RR)] = rrn; sc[mb(B_RHO1)] = rho1.re; sc[mb(B_RHO1) + 1] = rho1.im;
        if (half || rr < sc[mb(B_EPS)]) { sc[mb(B_DONE)] = 1.0; return; }
        if (!(fabs(rr) <= 1.79e308)) { sc[mb(B_DONE)] = 2.0; return; }      // NaN / inf: breakdown
        const c2 rho = {sc[mb(B_RHO)], sc[mb(B_RHO) + 1]}, al = {sc[mb(B_ALPHA)], sc[mb(B_ALPHA) + 1]}, om = {sc[mb(B_OMEGA)], sc[mb(B_OMEGA) + 1]};
        const c2 be = bicg_beta(rho1, rho, al, om);
        sc[mb(B_BETA)] = be.re; sc[mb(B_BETA) + 1] = be.im;
        sc[mb(B_RHO)] = rho1.re; sc[mb(B_RHO) + 1] = rho1.im;
    }
}

// ---------------------------------------------------------------------------------- streaming kernels: grid (nbk, n), the element arithmetic of bicgf_* (bicgstab_eo.hip)
// r = rhs - v (v == null: zero guess), r0 = p = r, |r|^2 partials
__global__ __launch_bounds__(UB) void mr_init(MrVec f, MrBuf b, int have_v, size_t n) {
    const int j = blockIdx.y;
    double2* __restrict__ r = pick12(f.r, j);
    double2* __restrict__ r0 = pick12(f.r0, j);
    double2* __restrict__ p = pick12(f.p, j);
    const double2* __restrict__ rhs = pick12(f.rhs, j);
    const double2* __restrict__ v = pick12(f.v, j);
    double acc[1] = {0};
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        const double2 bb = rhs[i], q = have_v ? v[i] : make_double2(0.0, 0.0);
        double2 o;
        o.x = bb.x - q.x; o.y = bb.y - q.y;
        r[i] = o; r0[i] = o; p[i] = o;
        acc[0] = fma(o.x, o.x, acc[0]); acc[0] = fma(o.y, o.y, acc[0]);
    }
    block_reduce_nv<1>(acc, b.P1 + (size_t)j * b.nbk);
}
// s = r - alpha v ; |s|^2 partials
__global__ __launch_bounds__(UB) void mr_s(MrVec f, MrBuf b, size_t n) {
    const int j = blockIdx.y;
    const double* sc = b.sc + (size_t)j * MR_NS;
    if (sc[mb(B_DONE)] != 0.0) return;
    double2* __restrict__ s = pick12(f.s, j);
    const double2* __restrict__ r = pick12(f.r, j);
    const double2* __restrict__ v = pick12(f.v, j);
    const double ar = sc[mb(B_ALPHA)], ai = sc[mb(B_ALPHA) + 1];
    double acc[1] = {0};
    for (size_t i = (size_t)blockIdx.x * UB + threadIdx.x; i < n; i += (size_t)gridDim.x * UB) {
        double2 sv = r[i];
        const double2 vv = v[i];
        sv.x = fma(-ar, vv.x, sv.x); sv.x = fma(ai, vv.y, sv.x);
        sv.y = fma(-ar, vv.y, sv.y); sv.y = fma(-ai, vv.x, sv.y);
        s[i] = sv;
        acc[0] = fma(sv.x, sv.x, acc[0]); acc[0] = fma(sv.y, sv.y, acc[0]);
    }
    block_reduce_nv<1>(acc, b.P1 + (size_t)j * b.nbk);
}
// x += alpha p + omega s ; r = s - omega t ; partials |r|^2, <r0, r>
__global__ __launch_bounds__(UB) void mr_xr(MrVec f, MrBuf b, size_t n) {
    const int j = blockIdx.y;
    const double* sc = b.sc + (size_t)j * MR_NS;
    if (sc[mb(B_DONE)] != 0.0) return;
    double2* __restrict__ x = pick12(f.x, j);
    double2* __restrict__ r = pick12(f.r, j);
    const double2* __restrict__ p = pick12(f.p, j);
    const double2* __restrict__ s = pick12(f.s, j);
    const double2* __restrict__ t = pick12(f.t, j);
    const double2* __restrict__ r0 = pick12(f.r0, j);
    const double ar = sc[mb(B_ALPHA)], ai = sc[mb(B_ALPHA) + 1], wr = sc[mb(B_OMEGA)], wi = sc[mb(B_OMEGA) + 1];
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
    block_reduce_nv<3>(acc, b.P3 + (size_t)j * 3 * b.nbk);
}
// p = r + beta (p - omega v)
__global__ __launch_bounds__(UB) void mr_p(MrVec f, MrBuf b, size_t n) {
    const int j = blockIdx.y;
    const double* sc = b.sc + (size_t)j * MR_NS;
    if (sc[mb(B_DONE)] != 0.0) return;
    double2* __restrict__ p = pick12(f.p, j);
    const double2* __restrict__ r = pick12(f.r, j);
    const double2* __restrict__ v = pick12(f.v, j);
    const double wr = sc[mb(B_OMEGA)], wi = sc[mb(B_OMEGA) + 1], br = sc[mb(B_BETA)], bi = sc[mb(B_BETA) + 1];
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

static int mr_block_get(lqcd_ctx_s* c, int nbs, int nbk, MrBuf& b) {
    const size_t per = (size_t)MR_NS + 6 * (size_t)nbs + 4 * (size_t)nbk, need = per * LQCD_MRHS_MAX;
    if (c->mrhs_block_n < need) {
        HIPCHK(hipStreamSynchronize(c->stream));
        (void)hipFree(c->mrhs_block);
        c->mrhs_block = nullptr; c->mrhs_block_n = 0;
        HIPCHK(hipMalloc((void**)&c->mrhs_block, need * sizeof(double)));
        c->mrhs_block_n = need;
    }
    b.nbs = nbs; b.nbk = nbk;
    b.sc = c->mrhs_block;
    b.P0 = b.sc + (size_t)LQCD_MRHS_MAX * MR_NS;
    b.P1 = b.P0 + (size_t)LQCD_MRHS_MAX * 3 * nbs;
    b.P2 = b.P1 + (size_t)LQCD_MRHS_MAX * nbk;
    b.P3 = b.P2 + (size_t)LQCD_MRHS_MAX * 3 * nbs;
    return LQCD_OK;
}

// x_j = D^-1 b_j (dagger: D^+) on FULL fields, j < n, with the multi-column hop.  status[j]: LQCD_OK or LQCD_ERR_NOT_CONVERGED
static int bicgstab_eo_wilson_mrhs(lqcd_op_s* op, int n, lqcd_spinor_s* const* x, lqcd_spinor_s* const* bsrc, int dg, double eps, int maxiter, int* iters, double* final_rr,
                                   int* status) {
    lqcd_ctx_s* c = op->ctx;
    const double k = op->km;
    const size_t nh = x[0]->elems / 2;
    ScratchScope pool(c);
    MrVec f = {};
    lqcd_spinor_s* to[LQCD_MRHS_MAX];
    double2* rhs[LQCD_MRHS_MAX];
    for (int j = 0; j < n; j++) {      // 8 half-fields per column
        lqcd_spinor_s* w[7];
        for (int q = 0; q < 7; q++) { w[q] = pool.get(LQCD_WILSON, LQCD_EVEN); if (!w[q]) return LQCD_ERR_HIP; }
        to[j] = pool.get(LQCD_WILSON, LQCD_ODD);
        if (!to[j]) return LQCD_ERR_HIP;
        f.r[j] = w[0]->data; f.r0[j] = w[1]->data; f.p[j] = w[2]->data; f.v[j] = w[3]->data; f.s[j] = w[4]->data; f.t[j] = w[5]->data;
        rhs[j] = w[6]->data; f.rhs[j] = rhs[j];
        f.x[j] = x[j]->data;
    }
    const int nbs = c->geom.Vh / 64;                                            // workgroups (= partials) of one dot hop
    const int nbk = (int)std::min<size_t>(1024, (nh + UB - 1) / UB);            // streaming kernels
    MrBuf b;
    LQCHK(mr_block_get(c, nbs, nbk, b));
    // out_j = in_j - k^2 H_eo H_oe in_j through to_j; z: the dot epilogue of the second hop; skip: the columns' done flags
    auto schur = [&](double2* const* out, double2* const* in, double2* const* z, double* dotp, int conj, bool skippable) -> int {
        MrhsCall h1, h2;
        h1.n = h2.n = n; h1.dagger = h2.dagger = dg;
        h1.parity_mode = 1; h1.a = 0.0; h1.b = 1.0;
        h2.parity_mode = 0; h2.a = 1.0; h2.b = -k * k;
        for (int j = 0; j < n; j++) {
            h1.out[1][j] = to[j]->data; h1.in[0][j] = in[j];
            h2.out[0][j] = out[j]; h2.in[1][j] = to[j]->data; h2.xin[0][j] = in[j];
            if (skippable) h1.done[j] = h2.done[j] = b.sc + (size_t)j * MR_NS + mb(B_DONE);
            if (z) { h2.dot_z[j] = z[j]; h2.dot_partial[j] = dotp + (size_t)j * 3 * nbs; }
        }
        h2.dot_conj = conj;
        LQCHK(mrhs_hop_launch(op, h1));
        return mrhs_hop_launch(op, h2);
    };
    // rhs_j = b_e + k H_eo b_o
    {
        MrhsCall h;
        h.n = n; h.dagger = dg; h.parity_mode = 0; h.a = 1.0; h.b = k;
        for (int j = 0; j < n; j++) { h.out[0][j] = rhs[j]; h.in[1][j] = bsrc[j]->data + nh; h.xin[0][j] = bsrc[j]->data; }
        LQCHK(mrhs_hop_launch(op, h));
    }
    const bool zero_guess = c->zero_guess_hint;      // the caller has just cleared every x: M x0 = 0 is not computed
    if (!zero_guess) LQCHK(schur(f.v, f.x, nullptr, nullptr, 0, false));
    const dim3 gk(nbk, n), gs(n);
    hipLaunchKernelGGL(mr_init, gk, dim3(UB), 0, c->stream, f, b, zero_guess ? 0 : 1, nh);
    hipLaunchKernelGGL(mr_init_scal, gs, dim3(MR_RB), 0, c->stream, b, eps);
    HIPCHK(hipGetLastError());
    std::vector<double> h((size_t)n * MR_NS, 0.0);
    bool all_done = false;
    int enq = 0;
    // the burst discipline of the single-column chain: the first burst runs up to what the last solve with this operator took (iterations enqueued behind a
    // column's converging one are no-ops for it), later bursts are short; one device-to-host copy of all columns' blocks per burst
    int check_every = std::max(4, std::min(op->bicg_mrhs_hint, 64));
    while (true) {
        const int burst = std::min(check_every, maxiter - enq);
        check_every = 2;
        for (int q = 0; q < burst; q++, enq++) {
            LQCHK(schur(f.v, f.p, f.r0, b.P0, 0, true));                                   // v = M p, <r0, v>
            hipLaunchKernelGGL(mr_step_alpha, gs, dim3(MR_RB), 0, c->stream, b);
            hipLaunchKernelGGL(mr_s, gk, dim3(UB), 0, c->stream, f, b, nh);
            LQCHK(schur(f.t, f.s, f.s, b.P2, 1, true));                                    // t = M s, <t, s>, |t|^2
            hipLaunchKernelGGL(mr_step_omega, gs, dim3(MR_RB), 0, c->stream, b);
            hipLaunchKernelGGL(mr_xr, gk, dim3(UB), 0, c->stream, f, b, nh);
            hipLaunchKernelGGL(mr_step_beta, gs, dim3(MR_RB), 0, c->stream, b);
            hipLaunchKernelGGL(mr_p, gk, dim3(UB), 0, c->stream, f, b, nh);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(h.data(), b.sc, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        all_done = true;
        for (int j = 0; j < n; j++) all_done = all_done && h[(size_t)j * MR_NS + mb(B_DONE)] != 0.0;
        if (all_done || enq >= maxiter) break;
    }
    // the odd halves (also on non-convergence, so every x is a consistent best effort): x_o = b_o + k H_oe x_e
    {
        MrhsCall ho;
        ho.n = n; ho.dagger = dg; ho.parity_mode = 1; ho.a = 1.0; ho.b = k;
        for (int j = 0; j < n; j++) { ho.out[1][j] = x[j]->data + nh; ho.in[0][j] = x[j]->data; ho.xin[1][j] = bsrc[j]->data + nh; }
        LQCHK(mrhs_hop_launch(op, ho));
    }
    int worst = LQCD_OK, itmax = 0;
    for (int j = 0; j < n; j++) {
        const double* sj = h.data() + (size_t)j * MR_NS;
        const int it = (int)sj[mb(B_ITERS)];
        if (iters) iters[j] = it;
        if (final_rr) final_rr[j] = sj[mb(B_RES)];
        itmax = std::max(itmax, it);
        status[j] = sj[mb(B_DONE)] == 1.0 ? LQCD_OK : LQCD_ERR_NOT_CONVERGED;
        if (status[j] != LQCD_OK && worst == LQCD_OK) {
            worst = LQCD_ERR_NOT_CONVERGED;
            if (sj[mb(B_DONE)] != 0.0) set_error("BiCGStab (column " + std::to_string(j) + "): residual is not finite (breakdown)");
            else set_error("The BiCGStab is not converged! column " + std::to_string(j) + ", maxsteps = " + std::to_string(maxiter) + ", residual = " + std::to_string(sj[mb(B_RES)]));
        }
    }
    if (worst == LQCD_OK) op->bicg_mrhs_hint = itmax;
    return worst;
}

// the argument checks the three entries share.  kind: 0 parity hop (opposite half-fields), 1 FULL fields
static int mrhs_check(lqcd_op_s* op, int n, const lqcd_spinor_t* out, const lqcd_spinor_t* in, int full, const char* who) {
    const std::string w(who);
    if (!(op && op->ctx && out && in)) { set_error(w + ": null argument"); return LQCD_ERR_ARG; }
    if (n < 1 || n > LQCD_MRHS_MAX) { set_error(w + ": 1 <= n <= LQCD_MRHS_MAX columns"); return LQCD_ERR_ARG; }
    for (int j = 0; j < n; j++)
        if (!out[j] || !in[j]) { set_error(w + ": null column"); return LQCD_ERR_ARG; }
    if (op->kind != LQCD_WILSON) { set_error(w + ": not available for the " + (op->kind == LQCD_STAGGERED ? "staggered" : "Domainwall") + " operator (Wilson and Wilson-clover only)"); return LQCD_ERR_UNSUPPORTED; }
    lqcd_ctx_s* c = op->ctx;
    if (!c->local_peers.empty()) { set_error(w + ": not available on an in-process PE grid"); return LQCD_ERR_UNSUPPORTED; }
    for (int j = 0; j < n; j++) {
        const lqcd_spinor_s *o = out[j], *i = in[j];
        if (o->ctx != c || i->ctx != c) { set_error(w + ": every field must belong to the operator's context"); return LQCD_ERR_ARG; }
        if (o->kind != LQCD_WILSON || i->kind != LQCD_WILSON || o->ls != 1 || i->ls != 1) { set_error(w + ": the columns must be four-dimensional Wilson fields"); return LQCD_ERR_ARG; }
        if (full) {
            if (o->subset != LQCD_FULL || i->subset != LQCD_FULL) { set_error(w + ": the columns must be FULL fields"); return LQCD_ERR_ARG; }
        } else {
            const bool opp = (o->subset == LQCD_EVEN && i->subset == LQCD_ODD) || (o->subset == LQCD_ODD && i->subset == LQCD_EVEN);
            if (!opp || o->subset != out[0]->subset) { set_error(w + ": out and in must be opposite parity subsets, the same for every column"); return LQCD_ERR_ARG; }
        }
        for (int q = 0; q < j; q++)
            if (out[q] == o || out[q]->data == o->data) { set_error(w + ": the output columns must be pairwise distinct"); return LQCD_ERR_ARG; }
    }
    for (int j = 0; j < n; j++)
        for (int q = 0; q < n; q++)
            if (out[j] == in[q] || out[j]->data == in[q]->data) { set_error(w + ": an output column is also an input column (inputs are never written)"); return LQCD_ERR_ARG; }
    return links_flush_of(op);      // the operator reads its links: recorded single-direction link operations run first (links.hip)
}

}  // namespace lqcd

using namespace lqcd;

extern "C" int lqcd_op_hop_multi(lqcd_op_t op, int n, const lqcd_spinor_t* out, const lqcd_spinor_t* in, int dagger) {
    LQCHK(mrhs_check(op, n, out, in, 0, "lqcd_op_hop_multi"));
    lqcd_ctx_s* c = op->ctx;
    if (!mrhs_applies(op)) {      // the single-column entry per column: its bits
        c->tun.mrhs_active = 0;
        for (int j = 0; j < n; j++) LQCHK(lqcd_op_hop(op, out[j], in[j], dagger));
        return LQCD_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    MrhsCall h;
    h.n = n; h.dagger = dagger ? 1 : 0; h.a = 0.0; h.b = 1.0;
    const int p = out[0]->subset == LQCD_EVEN ? 0 : 1;
    h.parity_mode = p;
    for (int j = 0; j < n; j++) { h.out[p][j] = out[j]->data; h.in[1 - p][j] = in[j]->data; }
    LQCHK(mrhs_hop_launch(op, h));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LQCD_OK;
}

extern "C" int lqcd_op_apply_multi(lqcd_op_t op, int n, const lqcd_spinor_t* out, const lqcd_spinor_t* in, int dagger) {
    LQCHK(mrhs_check(op, n, out, in, 1, "lqcd_op_apply_multi"));
    lqcd_ctx_s* c = op->ctx;
    if (!mrhs_applies(op)) {
        c->tun.mrhs_active = 0;
        for (int j = 0; j < n; j++) LQCHK(lqcd_op_apply(op, out[j], in[j], dagger));
        return LQCD_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    MrhsCall h;      // D = 1 - kappa H on both parities
    h.n = n; h.dagger = dagger ? 1 : 0; h.a = 1.0; h.b = -op->km; h.parity_mode = 2;
    for (int j = 0; j < n; j++)
        for (int p = 0; p < 2; p++) { h.out[p][j] = spinor_block(out[j], p); h.in[p][j] = spinor_block(in[j], p); h.xin[p][j] = spinor_block(in[j], p); }
    LQCHK(mrhs_hop_launch(op, h));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LQCD_OK;
}

extern "C" int lqcd_solve_bicgstab_eo_multi(lqcd_op_t op, int n, const lqcd_spinor_t* x, const lqcd_spinor_t* b, int dagger, double eps, int maxiter, int* iters,
                                            double* final_rr) {
    LQCHK(mrhs_check(op, n, x, b, 1, "lqcd_solve_bicgstab_eo_multi"));
    lqcd_ctx_s* c = op->ctx;
    if (!mrhs_applies(op)) {      // the single-column solver per column: its bits, its status (every column is attempted)
        c->tun.mrhs_active = 0;
        int worst = LQCD_OK;
        std::string msg;
        for (int j = 0; j < n; j++) {
            const int st = lqcd_solve_bicgstab_eo(op, x[j], b[j], dagger, eps, maxiter, iters ? iters + j : nullptr, final_rr ? final_rr + j : nullptr);
            if (st != LQCD_OK && st != LQCD_ERR_NOT_CONVERGED) return st;
            if (st != LQCD_OK && worst == LQCD_OK) { worst = st; msg = lqcd_last_error(); }
        }
        if (worst != LQCD_OK) set_error(msg);
        return worst;
    }
    HIPCHK(hipSetDevice(c->device));
    int status[LQCD_MRHS_MAX];
    const int st = bicgstab_eo_wilson_mrhs(op, n, x, b, dagger ? 1 : 0, eps, maxiter, iters, final_rr, status);
    hipError_t e = hipStreamSynchronize(c->stream);      // before the scratch fields go back to the pool
    if (e != hipSuccess && (st == LQCD_OK || st == LQCD_ERR_NOT_CONVERGED)) return hip_fail(e, "sync bicgstab_eo_multi", __FILE__, __LINE__);
    return st;
}
