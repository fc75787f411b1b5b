// wilsonloop.hip -- the R x T Wilson loops of the space-time planes, resident on the device.  Reference caller: the Wilson_loop measurement of the driver
// (src/measurements/measurement_parameters_set.jl:9-18, Measurement_set.jl:128-140 with Tmax = Rmax = 4) -> calc_Wilson_loop(U, Lt, Ls)
// (src/measurements/measure_Wilsonloop.jl:71-126): the loop [(mu, Ls), (4, Lt), (mu, -Ls), (4, -Lt)], mu = 1..3, real(WL) / NV / 3 / NC.
//
// Conventions (directions 0..3 = x, y, z, t; links periodic, no boundary sign, as lqcd_gauge_polyakov):
//   S_mu,R(x) = U_mu(x) U_mu(x + mu) ... U_mu(x + (R-1) mu)            mu = 0, 1, 2
//   T_T(x)    = U_3(x) U_3(x + t) ... U_3(x + (T-1) t)
//   W(R, T)   = 1/(9 V) sum_x sum_mu Re tr[ S_mu,R(x) T_T(x + R mu) S_mu,R(x + T t)^+ T_T(x)^+ ]
// Per R two sweeps and one small reduction, nothing synchronised with the host in between:
//   wl_extend_kernel   S_mu,R(x) = S_mu,R-1(x) U_mu(x + (R-1) mu) in place in one gauge-shaped temporary of the context (slots 0..2; R = 1 copies the links);
//                      a thread reads and writes its own site of S only, so the sweep needs no second buffer
//   wl_walk_kernel     one thread per (site, mu) holds S_mu,R(x), A = T_T(x) and B = T_T(x + R mu) in registers and steps T = 1..Tmax: two time-like links
//                      and S_mu,R(x + T t) per step (3 matrix loads = 432 B per (site, mu, T)), Re tr[(S B)(A S')^+]; no T-line field exists.  The sum of a
//                      step goes through the wave (shuffle tree), the block (LDS) and out as one block partial [T][mu][block]
//   wl_final_kernel    one block per T adds the 3 nblk partials of (R, T) in a fixed order (strided per thread, then a tree) into the device table
// One device-to-host copy of the Rmax x Tmax sums at the end; every order of summation is fixed, so a table is bitwise reproducible call to call.
// Partitioned lattices and in-process PE grids are refused (LQCD_ERR_UNSUPPORTED): the lines would cross ranks.
#include "lqcd_internal.h"
#include "gauge_staple.h"

#include <vector>

namespace lqcd {

constexpr int WL_THREADS = 256;

struct WLArgs {
    Geom g;
    const double2* U;
    double2* S;             // the line field: slots 0..2, slot 3 unused
    double* partial;        // [Tmax][3][nblk]
    int nblk, R, Tmax;
};

// site of thread t (the threads behind the last site take site 0 and contribute nothing)
__device__ __forceinline__ bool wl_site(const Geom& g, int& p, int& i, int (&x)[4]) {
    const int t = blockIdx.x * WL_THREADS + threadIdx.x;
    const bool act = t < 2 * g.Vh;
    const int s = act ? t : 0;
    p = s >= g.Vh ? 1 : 0;
    i = s - p * g.Vh;
    cb_to_coords(g, p, i, x);
    return act;
}

template <int MU>
__device__ __forceinline__ void wl_extend_dir(const WLArgs& k) {
    const Geom& g = k.g;
    int p, i, x[4];
    if (!wl_site(g, p, i, x)) return;
    const int Gs = glink_stride(g);
    x[MU] += k.R - 1;
    if (x[MU] >= g.L[MU]) x[MU] -= g.L[MU];
    cd u[9];
    load_m3(u, link_at(g, k.U, x, MU), Gs);
    double2* s = k.S + glink_off(g, p, MU, i);
    if (k.R == 1) { store_m3(s, Gs, u); return; }
    cd a[9], t[9];
    load_m3(a, s, Gs);
    mm3(t, a, u);
    store_m3(s, Gs, t);
}
__global__ __launch_bounds__(WL_THREADS) void wl_extend_kernel(WLArgs k) {
    if (blockIdx.y == 0) wl_extend_dir<0>(k);
    else if (blockIdx.y == 1) wl_extend_dir<1>(k);
    else wl_extend_dir<2>(k);
}

template <int MU>
__device__ __forceinline__ void wl_walk_dir(const WLArgs& k, double (&red)[2][WL_THREADS / 64]) {
    const Geom& g = k.g;
    int p, i, xa[4];
    const bool act = wl_site(g, p, i, xa);
    const int Gs = glink_stride(g);
    cd S[9], A[9], B[9], u[9], m[9], n[9];
    load_m3(S, k.S + glink_off(g, p, MU, i), Gs);
    int xb[4] = {xa[0], xa[1], xa[2], xa[3]};
    xb[MU] += k.R;
    if (xb[MU] >= g.L[MU]) xb[MU] -= g.L[MU];
#pragma unroll
    for (int e = 0; e < 9; e++) A[e] = B[e] = mk(e % 4 == 0 ? 1.0 : 0.0, 0.0);
#pragma unroll 1
    for (int T = 1; T <= k.Tmax; T++) {
        load_m3(u, link_at(g, k.U, xa, 3), Gs);         // U_t(x + (T-1) t)
        mm3(m, A, u);
#pragma unroll
        for (int e = 0; e < 9; e++) A[e] = m[e];
        load_m3(u, link_at(g, k.U, xb, 3), Gs);         // U_t(x + R mu + (T-1) t)
        mm3(m, B, u);
#pragma unroll
        for (int e = 0; e < 9; e++) B[e] = m[e];
        shift(xa, g, 3, 1);
        shift(xb, g, 3, 1);
        load_m3(u, link_at(g, k.S, xa, MU), Gs);        // S_mu,R(x + T t)
        mm3(m, S, B);
        mm3(n, A, u);
        double v = 0.0;                                 // Re tr[(S B)(A S')^+]
#pragma unroll
        for (int e = 0; e < 9; e++) v += m[e].re * n[e].re + m[e].im * n[e].im;
        v = shfl_tree_sum(act ? v : 0.0);
        const int b = T & 1;        // two LDS rows: thread 0 reads row b before the barrier of step T + 1, the writers of step T + 2 are behind it
        if ((threadIdx.x & 63) == 0) red[b][threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) k.partial[((size_t)(T - 1) * 3 + MU) * k.nblk + blockIdx.x] = (red[b][0] + red[b][1]) + (red[b][2] + red[b][3]);
    }
}
__global__ __launch_bounds__(WL_THREADS) void wl_walk_kernel(WLArgs k) {
    __shared__ double red[2][WL_THREADS / 64];
    if (blockIdx.y == 0) wl_walk_dir<0>(k, red);
    else if (blockIdx.y == 1) wl_walk_dir<1>(k, red);
    else wl_walk_dir<2>(k, red);
}

// out[T] = sum of partial[T][.], n values each, in a fixed order (strided per thread, then a tree)
__global__ __launch_bounds__(256) void wl_final_kernel(const double* __restrict__ partial, int n, double* __restrict__ out) {
    __shared__ double s[256];
    const double* q = partial + (size_t)blockIdx.x * n;
    double a = 0.0;
    for (int b = threadIdx.x; b < n; b += 256) a += q[b];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

static int wl_reserve(lqcd_ctx_s* c, double** buf, size_t* have, size_t n) {
    if (*have >= n) return LQCD_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)hipFree(*buf);
    *buf = nullptr; *have = 0;
    HIPCHK(hipMalloc((void**)buf, n * sizeof(double)));
    *have = n;
    return LQCD_OK;
}

}  // namespace lqcd

using namespace lqcd;

// the whole table of the Wilson_loop measurement: table[(R-1) Tmax + (T-1)] = W(R, T), R = 1..Rmax, T = 1..Tmax
extern "C" int lqcd_gauge_wilson_loops(lqcd_gauge_t U, int Rmax, int Tmax, double* table) {
    LQCHK(links_flush_of(U));
    ARGCHK(U && U->ctx && table, "lqcd_gauge_wilson_loops: null argument");
    lqcd_ctx_s* c = U->ctx;
    if (!c->local_peers.empty()) { set_error("lqcd_gauge_wilson_loops: not available on an in-process PE grid (the lines would cross domains)"); return LQCD_ERR_UNSUPPORTED; }
    if (any_partitioned(c)) { set_error("lqcd_gauge_wilson_loops: the lattice is partitioned (the lines would cross ranks)"); return LQCD_ERR_UNSUPPORTED; }
    const Geom& g = c->geom;
    const int Lmin = g.L[0] < g.L[1] ? (g.L[0] < g.L[2] ? g.L[0] : g.L[2]) : (g.L[1] < g.L[2] ? g.L[1] : g.L[2]);
    ARGCHK(Rmax >= 1 && Rmax <= Lmin && Tmax >= 1 && Tmax <= g.L[3], "lqcd_gauge_wilson_loops: 1 <= Rmax <= min(Lx, Ly, Lz) and 1 <= Tmax <= Lt");
    HIPCHK(hipSetDevice(c->device));
    const int nblk = (2 * g.Vh + WL_THREADS - 1) / WL_THREADS;
    const size_t ntab = (size_t)Rmax * Tmax;
    if (!c->wl_s) HIPCHK(hipMalloc((void**)&c->wl_s, U->elems * sizeof(double2)));
    LQCHK(wl_reserve(c, &c->wl_partial, &c->wl_partial_n, (size_t)3 * nblk * Tmax));
    LQCHK(wl_reserve(c, &c->wl_tab, &c->wl_tab_n, ntab));
    WLArgs k;
    k.g = g;
    k.U = U->data;
    k.S = c->wl_s;
    k.partial = c->wl_partial;
    k.nblk = nblk;
    k.Tmax = Tmax;
    for (int R = 1; R <= Rmax; R++) {
        k.R = R;
        hipLaunchKernelGGL(wl_extend_kernel, dim3(nblk, 3), dim3(WL_THREADS), 0, c->stream, k);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(wl_walk_kernel, dim3(nblk, 3), dim3(WL_THREADS), 0, c->stream, k);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(wl_final_kernel, dim3(Tmax), dim3(256), 0, c->stream, c->wl_partial, 3 * nblk, c->wl_tab + (size_t)(R - 1) * Tmax);
        HIPCHK(hipGetLastError());
    }
    std::vector<double> h(ntab);
    HIPCHK(hipMemcpyAsync(h.data(), c->wl_tab, ntab * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const double V = (double)c->gL[0] * c->gL[1] * c->gL[2] * c->gL[3];
    for (size_t j = 0; j < ntab; j++) table[j] = h[j] / (9.0 * V);
    return LQCD_OK;
}
