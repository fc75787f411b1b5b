// md.hip -- gauge side of the molecular-dynamics step on the device, the whole-field part: traceless anti-Hermitian momentum
// update, exponential link update, reunitarisation, momentum sampling and kinetic term, gauge action, Polyakov loop.  The staple force is staple.hip, the
// per-direction entry points and the recorder of their call triples links.hip, stout smearing stout.hip; shared device helpers: gauge_staple.h.
// Reference callers: P_update! / U_update! of the reference's src/md/AbstractMD.jl:78-118 (calc_dSdUmu!, Traceless_antihermitian_add!, exptU!),
// gauss_distribution!(p) src/md/standardMD.jl:86, action bookkeeping src/updates/standardHMC.jl:49-56.
// With lqcd_calc_UdSfdU (force.hip) a whole MD step runs without a host transfer: the links are uploaded once per trajectory.
//
// Conventions (the packages that own these generics are not vendored; these are fixed by dH/dtau = 0 and tested as such):
//   momenta P_mu(n): traceless anti-Hermitian 3x3 matrices in a gauge-shaped field, K = -sum tr P^2 (= p.p/2 for P = i p_a T_a);
//   dU/dtau = P U (U <- exp(dt P) U);   S_g = -(beta/3) sum_plaq Re tr U_p   (with rectangles: -(1/3) [beta_plaq sum_plaq + beta_rect sum_rect], rectangle.hip);
//   every force field G obeys dS/d eps [U -> exp(i eps T) U] = -2 Im tr(T G), hence dP/dtau = TA(G) = (G - G^+)/2 - tr(.)/3.
#include "lqcd_internal.h"
#include "gauge_staple.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace lqcd {

// P += c * TA(G)
__global__ __launch_bounds__(256) void momentum_add_ta_kernel(Geom g, double2* __restrict__ P, double cf, const double2* __restrict__ G) {
    size_t off;
    if (!link_of_thread(g, off)) return;
    const int Gs = glink_stride(g);
    cd m[9], a[9];
    load_m3(m, G + off, Gs);
    ta3(a, m, 0.5);
    // (the momenta are anti-Hermitian and so is the increment: the upper triangle is read, the lower one follows -- the same bits, see staple_links in staple.hip)
    cd o[9];
    auto addp = [&](auto E) {
        constexpr int e = decltype(E)::value;
        const cd pv = ld(P + off + (size_t)e * Gs);
        o[e] = mk(fma(cf, a[e].re, pv.re), fma(cf, a[e].im, pv.im));
    };
    addp(std::integral_constant<int, 0>()); addp(std::integral_constant<int, 1>()); addp(std::integral_constant<int, 2>());
    addp(std::integral_constant<int, 4>()); addp(std::integral_constant<int, 5>()); addp(std::integral_constant<int, 8>());
    o[3] = mk(-o[1].re, o[1].im); o[6] = mk(-o[2].re, o[2].im); o[7] = mk(-o[5].re, o[5].im);
#pragma unroll
    for (int e = 0; e < 9; e++) st(P + off + (size_t)e * Gs, o[e]);
}

template <bool REUNIT>
__global__ __launch_bounds__(256) void link_exp_update_kernel(Geom g, double2* __restrict__ U, double dt, const double2* __restrict__ P, unsigned* notproj) {
    size_t off;
    if (!link_of_thread(g, off)) return;
    const int Gs = glink_stride(g);
    cd x[9], e[9], t[9], u[9];
    load_m3(x, P + off, Gs);
    exp_m3(e, x, dt);
    load_m3(u, U + off, Gs);
    mm3(t, e, u);
    if constexpr (REUNIT) project_if_on_group(t, notproj);
#pragma unroll
    for (int k = 0; k < 9; k++) st(U + off + (size_t)k * Gs, t[k]);
}
__global__ __launch_bounds__(256) void link_reunitarize_kernel(Geom g, double2* __restrict__ U) {
    size_t off;
    if (!link_of_thread(g, off)) return;
    const int Gs = glink_stride(g);
    cd u[9];
    load_m3(u, U + off, Gs);
    reunitarize_m3(u);
#pragma unroll
    for (int k = 0; k < 9; k++) st(U + off + (size_t)k * Gs, u[k]);
}

__device__ inline void gauss2(uint64_t k, double& a, double& b) {
    const double u1 = u01(k), u2 = u01(splitmix64(k));
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
    sincos(6.283185307179586 * u2, &s, &c);
    a = r * c; b = r * s;
}
// P = i sum_a pi_a lambda_a / 2, pi_a ~ N(0,1) keyed by (seed, GLOBAL site, mu, a): identical for every decomposition
__global__ __launch_bounds__(256) void momentum_gaussian_kernel(Geom g, double2* __restrict__ P, uint64_t seed) {
    const int p = blockIdx.x & 1, i = (blockIdx.x >> 1) * 64 + (threadIdx.x & 63), mu = threadIdx.x >> 6;
    if (i >= g.Vh) return;
    int c[4];
    cb_to_coords(g, p, i, c);
    const uint64_t x = c[0] + g.origin[0], y = c[1] + g.origin[1], z = c[2] + g.origin[2], tt = c[3] + g.origin[3];
    const uint64_t gs = x + (uint64_t)g.gL[0] * (y + (uint64_t)g.gL[1] * (z + (uint64_t)g.gL[2] * tt));
    double pi[8];
    for (int a = 0; a < 4; a++) gauss2(rng_key(seed, gs * 4 + mu, 77, a), pi[2 * a], pi[2 * a + 1]);
    const double s3 = 0.5773502691896258;   // 1/sqrt(3)
    cd m[9];
    m[0] = mk(0.0, 0.5 * (pi[2] + s3 * pi[7]));
    m[4] = mk(0.0, 0.5 * (-pi[2] + s3 * pi[7]));
    m[8] = mk(0.0, -s3 * pi[7]);
    m[1] = mk(0.5 * pi[1], 0.5 * pi[0]);  m[3] = mk(-0.5 * pi[1], 0.5 * pi[0]);
    m[2] = mk(0.5 * pi[4], 0.5 * pi[3]);  m[6] = mk(-0.5 * pi[4], 0.5 * pi[3]);
    m[5] = mk(0.5 * pi[6], 0.5 * pi[5]);  m[7] = mk(-0.5 * pi[6], 0.5 * pi[5]);
    const size_t off = glink_off(g, p, mu, i);
    const int Gs = glink_stride(g);
#pragma unroll
    for (int e = 0; e < 9; e++) st(P + off + (size_t)e * Gs, m[e]);
}

// block partials of -Re tr P^2
__global__ __launch_bounds__(256) void momentum_action_kernel(Geom g, const double2* __restrict__ P, double* partial) {
    __shared__ double red[4];
    size_t off;
    double acc = 0.0;
    if (link_of_thread(g, off)) {
        const int Gs = glink_stride(g);
        cd m[9];
        load_m3(m, P + off, Gs);
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) acc -= m[a * 3 + b].re * m[b * 3 + a].re - m[a * 3 + b].im * m[b * 3 + a].im;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------------- Polyakov loop
// The second observable every trajectory of the reference's driver measures (measurement_methods Plaquette + Polyakov_loop in every test/*.toml;
// src/system/lqcd.jl:141 -> QCDMeasurements' Polyakov_measurement -> Gaugefields' calculate_Polyakov_loop(U, temp1, temp2)):
//     P = 1/(NC NX NY NZ) sum_x tr prod_{t = 0}^{NT-1} U_4(x, t)        [normalisation EXT-RECALL: the package's, as this file's author knows it]
// One thread per spatial site walks the time direction (links carry no boundary sign).  The time direction must not be partitioned.
__global__ __launch_bounds__(256) void polyakov_kernel(Geom g, const double2* __restrict__ U, double* __restrict__ partial) {
    const int V3 = g.L[0] * g.L[1] * g.L[2];
    const int s3 = blockIdx.x * 256 + threadIdx.x;
    double re = 0.0, im = 0.0;
    if (s3 < V3) {
        int c[4] = {s3 % g.L[0], (s3 / g.L[0]) % g.L[1], s3 / (g.L[0] * g.L[1]), 0};
        const int Gs = glink_stride(g);
        cd acc[9], u[9], t[9];
        load_m3(acc, link_at(g, U, c, 3), Gs);
        for (c[3] = 1; c[3] < g.L[3]; c[3]++) {
            load_m3(u, link_at(g, U, c, 3), Gs);
            mm3(t, acc, u);
#pragma unroll
            for (int e = 0; e < 9; e++) acc[e] = t[e];
        }
        re = acc[0].re + acc[4].re + acc[8].re;
        im = acc[0].im + acc[4].im + acc[8].im;
    }
    __shared__ double sh[2][4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { re += __shfl_down(re, off, 64); im += __shfl_down(im, off, 64); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = re; sh[1][threadIdx.x >> 6] = im; }
    __syncthreads();
    if (threadIdx.x < 2) partial[blockIdx.x * 2 + threadIdx.x] = (sh[threadIdx.x][0] + sh[threadIdx.x][1]) + (sh[threadIdx.x][2] + sh[threadIdx.x][3]);
}

// U <- exp(dt P) U enqueued on the context's stream; reunit: the projection rule of project_if_on_group, *notproj (device) is set when a link was left alone
int link_exp_update_enqueue(lqcd_gauge_s* U, double dt, const double2* P, bool reunit, unsigned* notproj) {
    lqcd_ctx_s* c = U->ctx;
    if (reunit) hipLaunchKernelGGL(link_exp_update_kernel<true>, dim3(link_grid(c->geom)), dim3(256), 0, c->stream, c->geom, U->data, dt, P, notproj);
    else hipLaunchKernelGGL(link_exp_update_kernel<false>, dim3(link_grid(c->geom)), dim3(256), 0, c->stream, c->geom, U->data, dt, P, notproj);
    HIPCHK(hipGetLastError());
    return LQCD_OK;
}
// U_update! (AbstractMD.jl:78-97) on the whole field, now (lqcd_gauge_exp_update and the recorder of links.hip decide when)
int gauge_exp_update_now(lqcd_gauge_t U, double dt, lqcd_gauge_t P) {
    lqcd_ctx_s* c = U->ctx;
    HIPCHK(hipSetDevice(c->device));
    U->version++;
    // md_reunitarize (default): an updated link that is unitary up to accumulated rounding (1e-13) is projected back onto SU(3) in the same
    // pass (links of a configuration that was never on the group to that precision are left alone).  exp(dt P) U leaves the group only by
    // rounding, but that rounding accumulates: max |row2 - conj(row0 x row1)| passes 1e-14 after ~280 updates (profiles/r03_unitarity_drift.log),
    // i.e. inside the FIRST trajectory, and the 12-real Dslash would be lost for the rest of the run.  0 = the reference's literal U_update!.
    const bool reunit = c->tun.md_reunitarize;
    bool all_projected;
    LQCHK(launch_with_notproj_flag(c, reunit, &all_projected, [&](unsigned* flag) { (void)link_exp_update_enqueue(U, dt, P->data, reunit, flag); }));
    if (all_projected) U->unitary_version = U->version;      // every link was projected: the field is on the group to rounding
    return LQCD_OK;
}

}  // namespace lqcd

using namespace lqcd;

extern "C" int lqcd_gauge_copy(lqcd_gauge_t dst, lqcd_gauge_t src) {      // substitute_U!(Uold, U) (standardHMC.jl:45)
    LQCHK(links_flush_of(dst));      // recorded single-direction link operations run first (links.hip)
    LQCHK(same_ctx(dst, src, "lqcd_gauge_copy"));
    lqcd_ctx_s* c = dst->ctx;
    HIPCHK(hipSetDevice(c->device));
    dst->version++;
    dst->unitary_version = src->unitary_version == src->version ? dst->version : 0;
    HIPCHK(hipMemcpyAsync(dst->data, src->data, src->elems * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LQCD_OK;
}

// S_g = -(beta/3) sum_plaq Re tr U_p = -beta * 6 V_global * plaquette
extern "C" int lqcd_gauge_action(lqcd_gauge_t U, double beta, double* Sg) {
    LQCHK(links_flush_of(U));      // recorded single-direction link operations run first (links.hip)
    ARGCHK(U && Sg, "lqcd_gauge_action: null argument");
    double plaq = 0;
    LQCHK(lqcd_gauge_plaquette(U, &plaq));
    const lqcd_ctx_s* c = U->ctx;
    *Sg = -beta * 6.0 * (double)c->gL[0] * c->gL[1] * c->gL[2] * c->gL[3] * plaq;
    return LQCD_OK;
}

// Traceless_antihermitian_add!(p, factor, G) (AbstractMD.jl:110,131):  P += factor * TA(G)
extern "C" int lqcd_momentum_add_ta(lqcd_gauge_t P, double factor, lqcd_gauge_t G) {
    LQCHK(links_flush_of(P));      // recorded single-direction link operations run first (links.hip)
    LQCHK(same_ctx(P, G, "lqcd_momentum_add_ta"));
    lqcd_ctx_s* c = P->ctx;
    HIPCHK(hipSetDevice(c->device));
    P->version++;
    hipLaunchKernelGGL(momentum_add_ta_kernel, dim3(link_grid(c->geom)), dim3(256), 0, c->stream, c->geom, P->data, factor, G->data);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return LQCD_OK;
}

// every link back onto SU(3) (Gram-Schmidt of rows 0, 1; row 2 = conj(row 0 x row 1)): for callers that update links through the
// single-direction entry points (the reference's own U_update!), once per trajectory keeps the 12-real Dslash path alive
extern "C" int lqcd_gauge_reunitarize(lqcd_gauge_t U) {
    LQCHK(links_flush_of(U));      // recorded single-direction link operations run first (links.hip)
    ARGCHK(U, "lqcd_gauge_reunitarize: null argument");
    lqcd_ctx_s* c = U->ctx;
    HIPCHK(hipSetDevice(c->device));
    U->version++;
    U->unitary_version = U->version;
    hipLaunchKernelGGL(link_reunitarize_kernel, dim3(link_grid(c->geom)), dim3(256), 0, c->stream, c->geom, U->data);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return LQCD_OK;
}

// gauss_distribution!(p) (standardMD.jl:86)
extern "C" int lqcd_momentum_gaussian(lqcd_gauge_t P, uint64_t seed) {
    LQCHK(links_flush_of(P));      // recorded single-direction link operations run first (links.hip)
    ARGCHK(P, "lqcd_momentum_gaussian: null argument");
    lqcd_ctx_s* c = P->ctx;
    HIPCHK(hipSetDevice(c->device));
    P->version++;
    hipLaunchKernelGGL(momentum_gaussian_kernel, dim3(link_grid(c->geom)), dim3(256), 0, c->stream, c->geom, P->data, seed);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return LQCD_OK;
}

// K = -sum tr P^2  (= md.p * md.p / 2, standardHMC.jl:49); summed over ranks
extern "C" int lqcd_momentum_action(lqcd_gauge_t P, double* K) {
    LQCHK(links_flush_of(P));      // recorded single-direction link operations run first (links.hip)
    ARGCHK(P && K, "lqcd_momentum_action: null argument");
    lqcd_ctx_s* c = P->ctx;
    HIPCHK(hipSetDevice(c->device));
    const int nb = link_grid(c->geom);
    ARGCHK(nb <= 2 * (2 * c->geom.Vh / 64 + 4096), "lqcd_momentum_action: partial buffer too small");
    hipLaunchKernelGGL(momentum_action_kernel, dim3(nb), dim3(256), 0, c->stream, c->geom, P->data, c->d_partial);
    HIPCHK(hipGetLastError());
    LQCHK(reduce_to_slot(c, nb, 1, S_RED0, true, 0));
    HIPCHK(hipMemcpyAsync(c->h_scal, c->d_scal + S_RED0, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *K = c->h_scal[0];
    return LQCD_OK;
}

extern "C" int lqcd_gauge_polyakov(lqcd_gauge_t U, double* re, double* im) {
    LQCHK(links_flush_of(U));
    ARGCHK(U && re && im, "lqcd_gauge_polyakov: null argument");
    lqcd_ctx_s* c = U->ctx;
    ARGCHK(!c->geom.part[3], "lqcd_gauge_polyakov: the time direction is partitioned (the loop would cross ranks)");
    ARGCHK(c->local_peers.empty(), "lqcd_gauge_polyakov: not available on an in-process PE grid");
    HIPCHK(hipSetDevice(c->device));
    const int V3 = c->geom.L[0] * c->geom.L[1] * c->geom.L[2], nb = (V3 + 255) / 256;
    ARGCHK(nb <= MAX_PARTIAL_BLOCKS, "lqcd_gauge_polyakov: partial buffer too small");
    hipLaunchKernelGGL(polyakov_kernel, dim3(nb), dim3(256), 0, c->stream, c->geom, U->data, c->d_partial);
    HIPCHK(hipGetLastError());
    LQCHK(reduce_to_slot(c, nb, 2, S_RED0, true, 0));
    HIPCHK(hipMemcpyAsync(c->h_scal, c->d_scal + S_RED0, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const double norm = 1.0 / (3.0 * (double)c->gL[0] * (double)c->gL[1] * (double)c->gL[2]);
    *re = norm * c->h_scal[0];
    *im = norm * c->h_scal[1];
    return LQCD_OK;
}
